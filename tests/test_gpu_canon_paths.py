"""Every canonical-graph builder on a real MI355X against the numpy restatements, row by row of tests/canon_cases.py
(which tests/test_canon_cases.py pins on the CPU): csrc/canon.hip (k_canon_build / _converse / _emit, the k_gen_* pipeline,
k_gen_pack, k_pair_relations), csrc/canon_small.hip and csrc/clevr_graph.hip at their word (64), block (256) and size
boundaries, on chains as long as the sample, on relations without an edge, with the `__image__` row anywhere.

Through the Python entries the datasets call.  Triplets, triplet_type, conv_counts and the counts the padding start implies
are integers: equality with the restatement, `T` included; nothing is computed from the device's output.  Before every run
the allocator's free blocks are filled with a non-zero pattern, so torch.empty workspaces and outputs hold garbage; every
row runs twice and must repeat bit for bit; every row runs with O = its longest sample and with O = 256 (poisoned padding
rows behind every sample either way)."""
import ctypes

import numpy as np
import pytest
import torch

import canon_cases as cc

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A
RUNNABLE = [r for r in cc.TABLE if not r["refused"]]
REFUSED = [r for r in cc.TABLE if r["refused"]]


def _dirty_fill():
    """Hand the caching allocator blocks of both pools filled with a non-zero pattern (tests/test_gpu_conv_plans.py does
    the same with NaN): what the next run allocates and does not write reads 0x5A bytes — a set bit in every word of a bit
    matrix, a huge count, an object index past every sample."""
    torch.cuda.synchronize()
    held = []
    for nbytes, count in ((4 << 10, 64), (64 << 10, 64), (512 << 10, 32), (2 << 20, 16), (16 << 20, 8), (64 << 20, 4)):
        held.extend(torch.full((nbytes // 8,), PATTERN, dtype=torch.int64, device="cuda") for _ in range(count))
    torch.cuda.synchronize()
    del held


def _run(row, path, O=None, uniforms="all", n_device=True):
    """One launch sequence of a row through the entry of `path` -> host arrays (triplets, conv_counts, triplet_type)."""
    from canonicalsg2im_amd.sg2im.data import annotated_triplets, canonical_triplets, clevr_triplets
    a = cc.inputs(row, O)
    vocab = a["vocab"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    objs, n = dev(a["objs"]), torch.from_numpy(a["n"])
    kw = dict(learned_transitivity=bool(row["trans"]), include_dummies=bool(row["dummies"]))
    if row["conv"]:
        u = a["uniforms"] if uniforms == "all" else None if uniforms is None else a["uniforms"][:uniforms]     # None: numpy's stream
        kw.update(learned_converse=True, converse_weights=a["weights"], uniforms=u)
    _dirty_fill()
    if path == "clevr":
        out = clevr_triplets(objs, n, vocab, dev(a["rel"]), rows_host=torch.from_numpy(a["rel"]), use_transitivity=row["trans"])
    elif path == "small" and row["vocab"] == "vg":     # the twin of a general_rows row: the same vocabulary, the small kernels
        out = annotated_triplets(objs, n, vocab, dev(a["rel"]), rows_host=torch.from_numpy(a["rel"]), **kw)
    elif path in ("small", "general_rows"):
        out = canonical_triplets(objs, None, None, n, vocab, triplets=torch.from_numpy(a["rel"]), **kw)
    elif path == "pairs":
        other, flip = torch.from_numpy(a["other"]), torch.from_numpy(a["flip"])
        out = canonical_triplets(objs, dev(a["boxes"]), dev(a["centers"]), n, vocab, pairs=(other.cuda(), flip.cuda()),
                                 pairs_host=(other, flip), use_converse=bool(row["use_converse"]), **kw)
    elif path == "general":
        rel = a["rel"] if row["annotated"] else np.zeros((len(n), 0, 3), np.int64)
        out = canonical_triplets(objs, dev(a["boxes"]), dev(a["centers"]), n, vocab, triplets=torch.from_numpy(rel), **kw)
    else:
        assert path == "lds" and len(vocab["pred_name_to_idx"]) == 8
        out = canonical_triplets(objs, dev(a["boxes"]), dev(a["centers"]), n.cuda() if n_device else n, vocab, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _same(got, want, row, what):
    t, conv, tt = got
    pad = cc.vocab_of(row)["pred_name_to_idx"]["__padding__"]
    assert t.dtype == np.int64 and tt.dtype == np.int64 and conv.dtype == np.float32, what
    assert t.shape == want["triplets"].shape, (what, t.shape, want["triplets"].shape)             # T is the oracle's
    assert np.array_equal(t, want["triplets"]), what
    assert np.array_equal(tt, want["tt"]), what
    assert conv.shape == want["conv"].shape and np.array_equal(conv, want["conv"]), what
    counts = want["counts"]
    for b in range(len(counts)):                        # the counts the padding start implies
        assert (t[b, counts[b]:] == [0, pad, 0]).all() and not tt[b, counts[b]:].any(), (what, b)
        assert not (t[b, :counts[b], 1] == pad).any(), (what, b)


@pytest.mark.parametrize("row", RUNNABLE, ids=[r["id"] for r in RUNNABLE])
def test_row_equals_the_restatement_and_itself(row):
    want = cc.expected(row)
    widths = sorted({max(row["sizes"]), 256 if cc.LIMIT[row["paths"][0]] == 256 else 80})
    first = None
    for path in row["paths"]:
        for O in widths:
            got = _run(row, path, O)
            what = "%s through %s at O = %d" % (row["id"], path, O)
            _same(got, want, row, what)
            if first is None:
                first = got
                print("%s: B = %d, T = %d, draws = %d, rows %s" % (row["id"], len(row["sizes"]), got[0].shape[1], want["draws"],
                                                                    want["counts"].tolist()))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first)), what      # lds == general, small == general_rows
        again = _run(row, path, widths[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first)), (row["id"], path, "second run")


@pytest.mark.parametrize("row", [r for r in RUNNABLE if r["conv"]], ids=[r["id"] for r in RUNNABLE if r["conv"]])
def test_the_uniform_numbers_consumed_are_the_oracles(row):
    """Fed exactly the oracle's number of draws the run succeeds with the oracle's answer; one fewer is the ValueError."""
    want = cc.expected(row)
    for path in row["paths"]:
        _same(_run(row, path, uniforms=want["draws"]), want, row, "%s through %s, exact uniforms" % (row["id"], path))
        if want["draws"] == 0:                          # a scene without a location row draws nothing: no number is needed
            assert row["family"] in ("identical", "single", "only_image")
            continue
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match="%d uniform numbers given, %d needed" % (want["draws"] - 1, want["draws"])):
            _run(row, path, uniforms=want["draws"] - 1)
        assert np.array_equal(np.random.get_state()[1], state)


def test_the_reversed_batch_gives_the_reversed_result():
    """No LDS or workspace state leaks from one block's sample to the next: (256, 1, 193, 2, 64, 256, 3) and its reverse."""
    for path in ("lds", "general"):
        a, b = _run(cc.ROWS["mixed"], path), _run(cc.ROWS["mixed_reversed"], path)
        assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0][::-1]) and np.array_equal(a[2], b[2][::-1])


@pytest.mark.parametrize("row", REFUSED, ids=[r["id"] for r in REFUSED])
def test_first_refused_size_and_rows_beyond_objs_are_refused(row):
    """257 rows (65 on the small kernels, 64 objects on the CLEVR ones) with the entry's existing message; n_objs[b] > O with
    ONE message on the location-only and the general path — with learned_converse on, before a uniform number is drawn,
    whether n_objs is on the host or on the device."""
    for path in row["paths"]:
        for n_device in ((True, False) if path == "lds" else (True,)):
            state = np.random.get_state()[1].copy()
            kw = {"uniforms": None} if row["conv"] else {}
            with pytest.raises(RuntimeError, match=row["refused"]):
                _run(row, path, n_device=n_device, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(np.random.get_state()[1], state), (row["id"], path)
    if row["n_over"]:                                   # the samples after it: the same batch with the count mended runs, and its
        mended = dict(row, id="lds_n_over_mended", n_over=None, refused=None)       # u_off are the oracle's (conv is on)
        want = cc.expected(mended)
        assert want["draws"] > 0 and (want["conv"][2].sum() > 0)
        for path in row["paths"]:
            _same(_run(mended, path, uniforms=want["draws"]), want, mended, "mended " + path)


# ------------------------------------------------------------------------------------------ the emit entries' `at < T` guard
GUARD = 4096


def _emit_checks(emit, counts, T0, what):
    """`emit(T, triplets, triplet_type)` over a built workspace whose longest sample — the LAST one, so that a row written
    past T lands in the guard — needs T0 rows: T0, then T0 - 1, 1 and 0, into sentinel-filled buffers of B * T rows and a
    guard region.  Rows below T equal the full emission's; every other word is the sentinel."""
    B = counts.shape[0]
    assert int(counts.sum(1).max()) == T0 == int(counts[-1].sum()) and T0 > 2
    full = None
    for T in (T0, T0 - 1, 1, 0):
        trip = torch.full((B * T * 3 + GUARD,), PATTERN, dtype=torch.int64, device="cuda")
        tt = torch.full((B * T + GUARD,), PATTERN, dtype=torch.int64, device="cuda")
        emit(T, trip, tt)
        torch.cuda.synchronize()
        assert bool((trip[B * T * 3:] == PATTERN).all()) and bool((tt[B * T:] == PATTERN).all()), (what, T)
        t, y = trip[:B * T * 3].view(B, T, 3).cpu(), tt[:B * T].view(B, T).cpu()
        if full is None:
            full = (t, y)
            assert not bool((t == PATTERN).any()) and not bool((y == PATTERN).any())       # every row was written
            assert int((y == 1).sum()) > 0                                                  # extras among them
        else:
            assert torch.equal(t, full[0][:, :T]) and torch.equal(y, full[1][:, :T]), (what, T)


def _emit_row():
    """(row, inputs): three samples, the longest last; transitive extras and dummies on."""
    row = dict(cc.ROWS["general_vg_permuted"], id="emit", sizes=(9, 3, 40), vocab="coco", permuted=0, annotated=False)
    return row, cc.inputs(row)


def test_csg_canon_emit_writes_nothing_at_or_beyond_T():
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    row, a = _emit_row()
    p2i = a["vocab"]["pred_name_to_idx"]
    objs, boxes, cen, n = (torch.from_numpy(a[k]).cuda() for k in ("objs", "boxes", "centers", "n"))
    B, O = objs.shape
    ids = (ctypes.c_int32 * 8)(*[p2i[k] for k in ("__padding__", "__in_image__") + tuple(cc_augmented())])
    nbytes = lib.csg_canon_workspace(B)
    ws = torch.full((nbytes // 8,), PATTERN, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 2), PATTERN, dtype=torch.int64, device="cuda")
    check(lib.csg_canon_build(ptr(objs), ptr(boxes), ptr(cen), ptr(n), B, O, ids, 0, 1, 1, ptr(ws), nbytes, ptr(counts), stream()),
          "canon_build")
    host = counts.cpu()
    want = cc.expected(dict(row, id="emit_lds", trans=1))
    assert host.sum(1).tolist() == want["counts"].tolist()

    def emit(T, trip, tt):
        check(lib.csg_canon_emit(ptr(objs), ptr(n), B, O, ids, 0, 1, 1, ptr(ws), ptr(counts), T, ptr(trip), ptr(tt), stream()),
              "canon_emit")

    _emit_checks(emit, host, int(want["counts"].max()), "csg_canon_emit")


def cc_augmented():
    from canonicalsg2im_amd.sg2im.data import augmented_relations
    return augmented_relations


def _roles(vocab):
    p2i = vocab["pred_name_to_idx"]
    roles = [-1] * len(p2i)
    roles[p2i["__padding__"]], roles[p2i["__in_image__"]] = -2, -3
    for slot, name in enumerate(cc_augmented()):
        roles[p2i[name]] = slot
    return (ctypes.c_int32 * len(roles))(*roles)


def test_csg_canon_general_emit_writes_nothing_at_or_beyond_T():
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    row, a = _emit_row()
    vocab = a["vocab"]
    P = len(vocab["pred_name_to_idx"])
    objs, boxes, cen = (torch.from_numpy(a[k]).cuda() for k in ("objs", "boxes", "centers"))
    n = np.ascontiguousarray(a["n"])
    B, O = objs.shape
    roles = _roles(vocab)
    nbytes = lib.csg_canon_general_workspace(B, P, 0)
    ws = torch.full(((nbytes + 7) // 8,), PATTERN, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 2), PATTERN, dtype=torch.int64, device="cuda")
    check(lib.csg_canon_general_build(ptr(objs), ptr(boxes), ptr(cen), n.ctypes.data_as(ctypes.c_void_p), B, O, None, None, 0,
                                      roles, P, 0, 1, ptr(ws), nbytes, ptr(counts), stream()), "general_build")
    check(lib.csg_canon_general_close(B, roles, P, 1, ptr(ws), nbytes, ptr(counts), stream()), "general_close")
    host = counts.cpu()
    want = cc.expected(dict(row, id="emit_lds", trans=1))
    assert host.sum(1).tolist() == want["counts"].tolist()

    def emit(T, trip, tt):
        check(lib.csg_canon_general_emit(B, roles, P, ptr(ws), nbytes, ptr(counts), T, ptr(trip), ptr(tt), stream()), "general_emit")

    _emit_checks(emit, host, int(want["counts"].max()), "csg_canon_general_emit")


def test_csg_canon_small_emit_writes_nothing_at_or_beyond_T():
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    row = dict(cc.ROWS["small_all"], id="emit_small", sizes=(9, 3, 40), conv=0, trans=1)
    a = cc.inputs(row)
    vocab = a["vocab"]
    p2i = vocab["pred_name_to_idx"]
    P = len(p2i)
    objs, rel_d = torch.from_numpy(a["objs"]).cuda(), torch.from_numpy(a["rel"]).cuda()
    n, rel = np.ascontiguousarray(a["n"]), np.ascontiguousarray(a["rel"])
    n_d = torch.from_numpy(n).cuda()
    B, O = objs.shape
    nbytes = lib.csg_canon_small_workspace(B, P)
    ws = torch.full(((nbytes + 7) // 8,), PATTERN, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 2), PATTERN, dtype=torch.int64, device="cuda")
    check(lib.csg_canon_small_build(ptr(objs), ptr(n_d), n.ctypes.data_as(ctypes.c_void_p), B, O, ptr(rel_d),
                                    rel.ctypes.data_as(ctypes.c_void_p), rel.shape[1], P, p2i["__padding__"], p2i["__in_image__"],
                                    vocab["object_name_to_idx"]["__image__"], 1, 1, None, None, None, 0, None, ptr(ws), nbytes,
                                    ptr(counts), stream()), "small_build")
    host = counts.cpu()
    want = cc.expected(row)
    assert host.sum(1).tolist() == want["counts"].tolist()

    def emit(T, trip, tt):
        check(lib.csg_canon_small_emit(B, P, p2i["__padding__"], ptr(ws), nbytes, ptr(counts), T, ptr(trip), ptr(tt), stream()),
              "small_emit")

    _emit_checks(emit, host, int(want["counts"].max()), "csg_canon_small_emit")
