"""The ADA augmentation pipeline on the device (csrc/ada_pipeline.hip): the table kernel against the host rows, the copy
paths as bits (identity rows, all 8 signed permutations x shifts against numpy's flip / rot90 / shift), the resampler's
weights as bits through one-hot inputs, its values and the adjoint against fp64 sums over those weights within the bounds
derived in tests/ada_pipeline_cases.py, the completeness of the adjoint's search, the colour matrix, the refusals, and the
policies inside the tiny trainer of tests/test_gpu_augment.py (`--use_img_disc 1` wherever bits are compared between two
trainers: the object discriminator's crop backward has float atomics).

The entries have no grid knob (one lane per float4, the grid follows from the shape), so there is no halved-grid case: the
adjoint's sum is ordered per source pixel by construction, and the second-run test holds the bits."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import ada_cases as ad
import ada_pipeline_cases as ap
import augment_cases as ac

pytestmark = pytest.mark.gpu

PAD = 64
ID_FLAGS = ap.GEOM_ID | ap.GEOM_INT | ap.COLOR_ID
SENT64 = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _dev(a, cuda):
    """A numpy float32 / int32 array on the device with its bits intact."""
    return torch.from_numpy(a.view(np.int32).copy()).to(cuda).view(torch.float32 if a.dtype == np.float32 else torch.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _launch(x, table, c0, cuda, bwd=False):
    """The C ABI entry on a buffer of our own, between two rows of sentinels.  x: (N, H, H, Ct) float32 (or its int32 bits)."""
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    x = np.ascontiguousarray(x).view(np.float32)
    N, H, _, Ct = x.shape
    table = np.ascontiguousarray(table, np.int32)
    assert table.shape == (table.shape[0], ap.ROW_WORDS)
    xd, td = _dev(x, cuda), _dev(table, cuda)
    buf = torch.full((2 * PAD + x.size,), int(ac.SENTINEL), dtype=torch.int32, device=cuda)
    out = buf[PAD:PAD + x.size].view(torch.float32)
    fn = lib.csg_ada_pipeline_bwd if bwd else lib.csg_ada_pipeline_fwd
    check(fn(ptr(xd), ptr(out), ptr(td), table.shape[0], N, H, Ct, c0, stream()), "ada_pipeline")
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == ac.SENTINEL).all() and (raw[PAD + x.size:] == ac.SENTINEL).all(), "a float outside the output was written"
    got = raw[PAD:PAD + x.size].view(np.float32).reshape(x.shape)
    return got


def _ctrl(cuda, p24):
    buf = torch.full((24,), SENT64, dtype=torch.int64, device=cuda)
    buf[8:16] = torch.tensor([int(p24), 3, 4, 5, 6, 7, 0, 0], dtype=torch.int64)
    return buf, buf[8:16]


def _generated(cuda, rows, H, policy=56, p24=ap.ONE, key=(21, 4, 1, 0)):
    """Rows read back from the device's table kernel."""
    from canonicalsg2im_amd import ops
    _, ctrl = _ctrl(cuda, p24)
    return ops.ada_pipeline_table(key[0], key[1], key[2], rows, H, policy, ctrl, rank=key[3]).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the table kernel
@pytest.mark.parametrize("H", [5, 8, 16, 256])
def test_table_kernel_equals_the_host_rows(H, cuda):
    from canonicalsg2im_amd import ops
    rows = 70
    for seed, iteration, pass_id, rank in ap.KEYS:
        for p24 in ap.P24_VALUES:
            for policy in (8, 16, 32, 56):
                buf, ctrl = _ctrl(cuda, p24)
                got = ops.ada_pipeline_table(seed, iteration, pass_id, rows, H, policy, ctrl, rank=rank).cpu().numpy()
                want = ops.ada_pipeline_table_host(seed, iteration, pass_id, rows, H, policy, p24, rank=rank).numpy()
                bad = np.argwhere(got != want)
                assert bad.size == 0, (H, p24, policy, bad[:4].tolist())
                raw = buf.cpu().tolist()
                assert raw[:8] == [SENT64] * 8 and raw[16:] == [SENT64] * 8 and raw[8:16] == [p24, 3, 4, 5, 6, 7, 0, 0]
    # `out`: the rows asked for and no word beyond; a p24 outside [0, 2^24] is clamped (the launch cannot refuse what it reads)
    out = torch.full((12, 32), 77, dtype=torch.int32, device=cuda)
    _, ctrl = _ctrl(cuda, 1 << 40)
    ops.ada_pipeline_table(1, 2, 0, 8, H, 56, ctrl, out=out)
    assert np.array_equal(out[:8].cpu().numpy(), ops.ada_pipeline_table_host(1, 2, 0, 8, H, 56, ap.ONE).numpy())
    assert bool((out[8:] == 77).all())
    _, ctrl = _ctrl(cuda, -5)
    assert bool((ops.ada_pipeline_table(1, 2, 0, 8, H, 56, ctrl)[:, 13] == ID_FLAGS).all())


# ------------------------------------------------------------------------------------------------ 2. the copy paths
@pytest.mark.parametrize("shape", [(3, 5, 4, 0), (2, 8, 8, 5), (2, 16, 12, 3), (64, 9, 4, 1)], ids=lambda s: "N%d_H%d_Ct%d_c%d" % s)
def test_identity_rows_are_bit_copies(shape, cuda):
    """-0.0, infinities, NaN payloads and denormals go through unchanged, forward and adjoint, whatever M, G and C hold: the
    flags alone select the path.  The rows of a p = 0 table are such rows."""
    N, H, Ct, c0 = shape
    x = ap.special_values((N, H, H, Ct), 11)
    junk = ap.make_row(H, (np.nan, 3.0, -2.0, np.inf), (1e30, -7.0), flags=ID_FLAGS, colour=[np.nan] * 12,
                       intmap=(5, 5, 5, 5, 9, 9), G=(np.nan,) * 6)
    for table in (np.stack([junk] * N), _generated(cuda, N, H, p24=0)):
        for bwd in (False, True):
            got = _launch(x, table, c0, cuda, bwd=bwd)
            assert np.array_equal(_bits(got), x), (shape, bwd)


@pytest.mark.parametrize("H", [8, 5])
def test_blit_rows_are_numpy_flip_rot90_shift(H, cuda):
    """All 8 signed permutations x 8 shifts (0, +-1, +-t_max, beyond +-H) in one launch of 64 samples: the output's bits are
    numpy's flip / rot90 / zero-filled shift, the adjoint's bits the inverse sequence."""
    cases = [(f, k, tx, ty) for f, k in ap.SIGNED_PERMUTATIONS for tx, ty in ap.blit_shifts(H)]
    assert len(cases) == 64
    table = np.stack([ap.make_row(H, (np.nan,) * 4, flags=ap.GEOM_INT | ap.COLOR_ID, intmap=ap.blit_map(f, k, tx, ty, H))
                      for f, k, tx, ty in cases])
    x = ac.data((64, H, 8, 0), 5)
    fwd, bwd = _launch(x, table, 2, cuda), _launch(x, table, 2, cuda, bwd=True)
    for n, (f, k, tx, ty) in enumerate(cases):
        assert np.array_equal(_bits(fwd[n]), _bits(ap.blit_np(x[n], f, k, tx, ty))), (n, f, k, tx, ty)
        assert np.array_equal(_bits(bwd[n]), _bits(ap.blit_adjoint_np(x[n], f, k, tx, ty))), (n, f, k, tx, ty)
    # what is not a signed permutation gives zeros, whatever it is
    bad = np.stack([ap.make_row(H, flags=ap.GEOM_INT | ap.COLOR_ID, intmap=m)
                    for m in ((1, 1, 0, 1, 0, 0), (2, 0, 0, 1, 0, 0), (1, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0),
                              (1 << 30, 0, 0, -(1 << 31), 0, 0), (1, 0, 0, 1, (1 << 31) - 1, -(1 << 31)))])
    for b in (False, True):
        assert not _bits(_launch(x[:6], bad, 2, cuda, bwd=b)).any()


def test_generated_blit_rows_are_their_draws(cuda):
    """The device's own blit-only rows at p = 1 and p = 1/2 do to a picture what the restated draws say, through numpy."""
    for H in (8, 9):
        for p24 in (ap.ONE, 1 << 23):
            key = (3, 6, 2, 1)
            table = _generated(cuda, 48, H, policy=ap.BLIT, p24=p24, key=key)
            flip, k, tx, ty, _ = ap.blit_draws(ap.key_np(key[0], key[1], key[2], key[3], 48), H, p24)
            x = ac.data((48, H, 4, 0), 6)
            got = _launch(x, table, 0, cuda)
            for n in range(48):
                assert np.array_equal(_bits(got[n]), _bits(ap.blit_np(x[n], bool(flip[n]), int(k[n]), int(tx[n]), int(ty[n])))), (H, n)


# ------------------------------------------------------------------------------------------------ 3. the resampler
def _rows_for(cuda, H):
    rows = dict(ap.hand_rows(H))
    gen = _generated(cuda, 32, H, policy=ap.BLIT | ap.GEOM, p24=ap.ONE)
    assert (gen[:, 13] == ap.COLOR_ID).all()
    rows.update({"generated_%d" % i: r for i, r in enumerate(gen)})
    return rows


@pytest.fixture(scope="module")
def rows8(cuda):
    return _rows_for(cuda, 8)


def _one_hot(H, Ct, ch):
    x = np.zeros((H * H, H, H, Ct), np.float32)
    i = np.arange(H * H)
    x[i, i // H, i % H, ch] = 1.0
    return x


def _check_weights(row, H, cuda, name):
    """Sample i holds a single 1 at pixel i.  Forward: output pixel p of sample i is the weight of source i in p.  Adjoint:
    source pixel q of sample i is the weight of q in output i — and 0 wherever q is no tap of i: a candidate the walk missed
    leaves a 0 where the forward has a weight, a tap met twice doubles it."""
    W, tap = ap.weight_matrix(row, H)
    x = _one_hot(H, 4, 1)
    table = np.stack([row] * (H * H))
    fwd = _launch(x, table, 0, cuda)[..., 1].reshape(H * H, H * H)           # [source i, output p]
    assert np.array_equal(_bits(fwd), _bits(W.T.copy())), "%s: a forward weight differs in its bits" % name
    bwd = _launch(x, table, 0, cuda, bwd=True)
    assert not _bits(bwd[..., [0, 2, 3]]).any(), name
    bwd = bwd[..., 1].reshape(H * H, H * H)                                   # [output i, source q]
    missed = int(((bwd == 0) & (W != 0)).sum())
    assert np.array_equal(_bits(bwd), _bits(W)), "%s: the adjoint differs from the forward's weights (%d taps missed)" % (name, missed)
    return W, tap


def test_weights_and_the_adjoints_search_H8(rows8, cuda):
    """H = 8, N = 64: every hand-made row and 32 generated ones (blit and geometry on at p = 1)."""
    for name, row in rows8.items():
        W, tap = _check_weights(row, 8, cuda, name)
        if name in ap.ZERO_ROWS:
            assert not tap.any(), name
        if name in ("on_integers", "half_pixel"):
            print(name, "taps per output:", sorted(set(tap.sum(1).tolist())))
    W, _ = ap.weight_matrix(rows8["on_integers"], 8)
    assert np.array_equal(W, np.eye(64, dtype=np.float32))                   # fx = 0 everywhere, x0 + 1 = H at the edge
    assert ap.weight_matrix(rows8["mag4"], 8)[1].sum(0).max() >= 16          # a source pixel held by 16 or more outputs
    sides = [ap.box_side_bound(r) for n, r in rows8.items() if n not in ap.ZERO_ROWS]
    print("largest box side %d" % max(sides))
    assert max(sides) <= ap.MAX_BOX


def test_weights_and_the_adjoints_search_odd_centre(cuda):
    """H = 5: the centre (H - 1) / 2 is a whole number."""
    for name, row in _rows_for(cuda, 5).items():
        _check_weights(row, 5, cuda, name)


@pytest.mark.parametrize("H", [8, 9, 16])
def test_values_and_adjoint_within_the_bounds(H, cuda):
    rng = np.random.default_rng(40 + H)
    for name, row in _rows_for(cuda, H).items():
        W, tap = ap.weight_matrix(row, H)
        W64 = W.astype(np.float64)
        x = ac.data((3, H, 8, 0), 50 + H)
        table = np.stack([row] * 3)
        got = _launch(x, table, 0, cuda).reshape(3, H * H, 8)
        ref = np.einsum("pq,nqc->npc", W64, x.reshape(3, H * H, 8).astype(np.float64))
        bound = ap.INTERP_ROUNDINGS * ap.U * np.abs(x).max() * ap.SLACK
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= bound, "%s: forward error %.3g, bound %.3g" % (name, err, bound)
        if name in ap.ZERO_ROWS:
            assert not _bits(got).any(), name
        g = rng.uniform(-1.0, 1.0, size=(3, H, H, 8)).astype(np.float32)
        got = _launch(g, table, 0, cuda, bwd=True).reshape(3, H * H, 8)
        g64 = g.reshape(3, H * H, 8).astype(np.float64)
        ref = np.einsum("pq,npc->nqc", W64, g64)
        S = np.einsum("pq,npc->nqc", W64, np.abs(g64))
        terms = tap.sum(0)[None, :, None]
        bound = (terms + ap.TERM_ROUNDINGS) * ap.U * S * ap.SLACK
        bad = np.abs(got.astype(np.float64) - ref) > bound
        assert not bad.any(), "%s: %d adjoint values beyond the bound, e.g. %s" % (name, int(bad.sum()), np.argwhere(bad)[0])
        assert not _bits(got)[np.broadcast_to(terms == 0, got.shape)].any(), name


def test_foreign_forward_maps_give_an_empty_walk(cuda):
    for name, row in ap.foreign_rows(8).items():
        g = ac.data((2, 8, 4, 0), 3)
        assert not _bits(_launch(g, np.stack([row] * 2), 0, cuda, bwd=True)).any(), name
        assert np.array_equal(_launch(g, np.stack([row] * 2), 0, cuda), g), name      # M is the identity (values: w * -0.0 + 0.0 = +0.0)


# ------------------------------------------------------------------------------------------------ 4. the colour matrix
@pytest.mark.parametrize("shape", [(2, 5, 4, 0), (2, 8, 4, 1), (3, 8, 8, 3), (2, 9, 8, 5), (2, 8, 12, 5), (2, 16, 12, 9)],
                         ids=lambda s: "N%d_H%d_Ct%d_c%d" % s)
def test_colour_matrix(shape, cuda):
    """Identity geometry, hand-made and generated matrices: the triple inside one float4 (c0 % 4 < 2) and straddling two."""
    N, H, Ct, c0 = shape
    rng = np.random.default_rng(sum(shape))
    gen = _generated(cuda, N, H, policy=ap.COLOR, p24=ap.ONE)
    assert (gen[:, 13] == (ap.GEOM_ID | ap.GEOM_INT)).all()
    hand = np.stack([ap.make_row(H, flags=ap.GEOM_ID | ap.GEOM_INT, colour=ap.random_colour(rng)) for _ in range(N)])
    x = ac.data((N, H, Ct, 0), 9)
    other = [c for c in range(Ct) if not c0 <= c < c0 + 3]
    for table in (hand, gen):
        for bwd, fn, k in ((False, ap.colour_fwd, ap.COLOR_ROUNDINGS), (True, ap.colour_bwd, ap.COLOR_ADJOINT_ROUNDINGS)):
            got = _launch(x, table, c0, cuda, bwd=bwd)
            assert np.array_equal(_bits(got[..., other]), _bits(x[..., other])), "a channel outside the triple was touched"
            for n in range(N):
                ref, L = fn(x[n][..., c0:c0 + 3].astype(np.float64), table[n])
                err = np.abs(got[n][..., c0:c0 + 3].astype(np.float64) - ref).max()
                assert err <= k * ap.U * L, (shape, bwd, n, err, k * ap.U * L)


def test_colour_after_the_resampling(cuda):
    """Geometry and colour together: the matrix acts on the interpolated triple — a zero-filled pixel takes the offset —, and
    the adjoint is the transpose: <A x - A 0, g> = <x, A^T g> in fp64 to the roundings of both sides."""
    H, Ct, c0, N = 9, 8, 3, 4
    rng = np.random.default_rng(8)
    names = ("rot45", "half_pixel", "out_right", "mag4")
    table = np.stack([ap.make_row(H, flags=0, colour=ap.random_colour(rng)) for _ in names])
    for i, name in enumerate(names):
        table[i, 0:13] = ap.hand_rows(H)[name][0:13]
    x = ac.data((N, H, Ct, 0), 12)
    got = _launch(x, table, c0, cuda)
    zero = _launch(np.zeros_like(x), table, c0, cuda)
    g = rng.uniform(-1.0, 1.0, size=x.shape).astype(np.float32)
    gin = _launch(g, table, c0, cuda, bwd=True)
    tol = 0.0
    for n, name in enumerate(names):
        W64 = ap.weight_matrix(table[n], H)[0].astype(np.float64)
        v = (W64 @ x[n].reshape(H * H, Ct).astype(np.float64)).reshape(H, H, Ct)
        ref, L = ap.colour_fwd(v[..., c0:c0 + 3], table[n])
        C = ap.colour_of(table[n])
        interp = ap.INTERP_ROUNDINGS * ap.U * np.abs(x[n]).max() * ap.SLACK
        rs = np.abs(C[:, :3]).sum(1).max()                  # the interpolation's error goes through the matrix: <= rs * interp
        bound = ap.COLOR_ROUNDINGS * ap.U * (L + rs * interp) + rs * interp
        assert np.abs(got[n][..., c0:c0 + 3].astype(np.float64) - ref).max() <= bound, name
        # the dot-product test's tolerance: |g| times the forward's bound, |x| times the adjoint's — (terms + 1 + 5) roundings
        # of magnitudes up to S' = W^T (|C|^T |g|)
        T = np.abs(g[n].astype(np.float64)).reshape(H * H, Ct)
        T[:, c0:c0 + 3] = T[:, c0:c0 + 3] @ np.abs(C[:, :3])
        terms = ap.weight_matrix(table[n], H)[1].sum(0)[:, None]
        adj = (terms + ap.TERM_ROUNDINGS + ap.COLOR_ADJOINT_ROUNDINGS) * ap.U * (W64.T @ T) * ap.SLACK
        tol += np.abs(g[n]).sum() * max(bound, interp) + (np.abs(x[n].astype(np.float64)).reshape(H * H, Ct) * adj).sum()
        assert np.array_equal(_bits(zero[n][..., c0:c0 + 3]), _bits(np.broadcast_to(C[:, 3].astype(np.float32), (H, H, 3)))), name
    assert not _bits(got[2][..., [0, 1, 2, 6, 7]]).any()                      # out_right: zero fill outside the triple
    lhs = ((got.astype(np.float64) - zero.astype(np.float64)) * g).sum()
    rhs = (x.astype(np.float64) * gin.astype(np.float64)).sum()
    print("<A x - A 0, g> = %.9g, <x, A^T g> = %.9g, tolerance %.3g" % (lhs, rhs, 2 * tol))
    assert abs(lhs - rhs) <= 2 * tol, (lhs, rhs, tol)                                  # (2: A 0 carries the forward's error too)


# ------------------------------------------------------------------------------------------------ 5. the entries
def test_two_launches_give_the_same_bits(cuda):
    table = _generated(cuda, 8, 16)
    x = ac.data((8, 16, 12, 0), 31)
    for bwd in (False, True):
        a, b = _launch(x, table, 5, cuda, bwd=bwd), _launch(x, table, 5, cuda, bwd=bwd)
        assert np.array_equal(_bits(a), _bits(b)) and np.isfinite(a).all()


def test_autograd_through_ops(cuda):
    from canonicalsg2im_amd import ops
    table = _generated(cuda, 3, 16)
    x = ac.data((3, 16, 8, 0), 32)
    g = ac.data((3, 16, 8, 0), 33)
    xd = _dev(x, cuda).permute(0, 3, 1, 2).requires_grad_(True)              # logical NCHW, NHWC memory
    td = _dev(table, cuda)
    y = ops.ada_pipeline(xd, td, 4)
    assert y.shape == xd.shape and np.array_equal(_bits(y.detach().permute(0, 2, 3, 1).cpu().numpy()), _bits(_launch(x, table, 4, cuda)))
    y.backward(_dev(g, cuda).permute(0, 3, 1, 2))
    assert np.array_equal(_bits(xd.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy()), _bits(_launch(g, table, 4, cuda, bwd=True)))
    for bad, what in ((dict(c0=6), "c0 \\+ 3 > Ct"), (dict(table=td[:2]), "fewer than N = 3"), (dict(table=td.view(-1, 8)), "int32 \\(rows, 32\\)"),
                      (dict(table=td.cpu()), "the table is on")):
        a = dict(dict(table=td, c0=4), **bad)
        with pytest.raises(RuntimeError, match=what):
            ops.ada_pipeline(xd, a["table"], a["c0"])
    with pytest.raises(RuntimeError, match="Ct % 4"):
        ops.ada_pipeline(xd[:, :6], td, 0)
    with pytest.raises(RuntimeError, match="policy must be a mask"):
        ops.ada_pipeline_table(0, 0, 0, 2, 8, 64, _ctrl(cuda, 0)[1])


def test_library_refusals(cuda):
    from canonicalsg2im_amd._lib import last_error, lib, ptr, stream
    x = torch.ones((2, 4, 4, 8), device=cuda)
    sent = torch.full((2, 4, 4, 8), 3.0, device=cuda)
    table = torch.zeros((3, 32), dtype=torch.int32, device=cuda)
    off4 = ctypes.c_void_p(table.data_ptr() + 4)
    for fn in (lib.csg_ada_pipeline_fwd, lib.csg_ada_pipeline_bwd):
        for args, what in (((ptr(x), ptr(x), ptr(table), 3, 2, 4, 8, 0), "not in place"), ((ptr(x), ptr(sent), ptr(table), 3, 2, 4, 6, 0), "multiple of 4"),
                           ((ptr(x), ptr(sent), ptr(table), 3, 2, 4, 8, 6), "c0 + 3 > Ct"), ((ptr(x), ptr(sent), off4, 3, 2, 4, 8, 0), "16-byte aligned"),
                           ((ptr(x), ptr(sent), ptr(table), 1, 2, 4, 8, 0), "fewer than N = 2"), ((ptr(x), ptr(sent), None, 3, 2, 4, 8, 0), "null pointer"),
                           ((ptr(x), ptr(sent), ptr(table), 3, 2, 1, 8, 0), "H = 1"), ((ptr(x), ptr(sent), ptr(table), 3, 2, 4, 8, -1), "c0 + 3 > Ct")):
            assert fn(*args, stream()) != 0 and what in last_error(), (what, last_error())
    _, ctrl = _ctrl(cuda, 5)
    off = ctypes.c_void_p(ctrl.data_ptr() + 4)
    for args, what in (((0, 0, 0, 0, 3, 8, 56, None, ptr(table)), "null pointer"), ((0, 0, 0, 0, 3, 8, 56, off, ptr(table)), "misaligned"),
                       ((0, 0, 0, 0, 3, 8, 56, ptr(ctrl), off4), "16-byte aligned"), ((0, 0, 0, 0, 3, 8, 56, ptr(ctrl), None), "null pointer"),
                       ((0, 0, 0, 0, 3, 8, 64, ptr(ctrl), ptr(table)), "policy 64"), ((0, 0, 0, 0, 3, 1, 56, ptr(ctrl), ptr(table)), "H = 1"),
                       ((0, 0, -1, 0, 3, 8, 56, ptr(ctrl), ptr(table)), "non-negative"), ((0, 0, 0, 0, 1 << 27, 8, 56, ptr(ctrl), ptr(table)), "rows")):
        assert lib.csg_ada_pipeline_table(*args, stream()) != 0 and what in last_error(), (what, last_error())
    torch.cuda.synchronize()
    assert bool((sent == 3.0).all()) and not bool(table.any())


# ------------------------------------------------------------------------------------------------ 6. the trainer
TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2", "--learning_rate", "5e-3"]
ADA = "ada_blit,ada_geom,ada_color"
HALF = ["--d_augment_p", "0.5"]
STEPS = 4


def _make(cuda, graphs, policies=ADA, flags=HALF, seed=0, extra=("--use_img_disc", "1")):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY + list(extra) + ["--d_augment", policies] + list(flags))
    torch.manual_seed(seed)
    tr = T.Trainer(opt, cuda)
    if not graphs:
        tr.graphs = None
    else:
        assert tr.graphs is not None, "graph replay should be available for this recipe"
    return vocab, tr


def _batch(vocab, cuda, seed, B=2):
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    return [None if t is None else t.to(cuda) for t in make_batch(vocab, BatchConfig(B, 64, 2, 5, "packed"), seed)]


def _step(tr, batch, n):
    torch.manual_seed(1000 + n)
    G, D = tr.step(batch)
    return {k: v.clone() for k, v in G.items()}, {k: v.clone() for k, v in D.items()}


def _weights(tr):
    return [(n, p.detach().clone()) for n, p in list(tr.model.named_parameters()) + list(tr.discriminator.named_parameters())]


def _assert_same_run(a, b, what):
    assert len(a) == len(b)
    for n, ((Ga, Da), (Gb, Db)) in enumerate(zip(a, b), 1):
        assert list(Ga) == list(Gb) and list(Da) == list(Db)
        for k in list(Ga) + list(Da):
            x, y = (Ga[k], Gb[k]) if k in Ga else (Da[k], Db[k])
            assert _same_bits(x, y), "%s: %s of step %d: %r against %r" % (what, k, n, x.flatten()[:3].tolist(), y.flatten()[:3].tolist())


def _assert_same_weights(a, b, what):
    diff = [n for (n, x), (_, y) in zip(a, b) if not _same_bits(x, y)]
    assert not diff, "%s: %d tensors differ, e.g. %s" % (what, len(diff), diff[:3])


@pytest.fixture(scope="module")
def eager_run(cuda):
    """Four eager steps with the three ADA groups at p = 1/2; the persistent rows after every step; a checkpoint after step 2."""
    from canonicalsg2im_amd import ops
    vocab, tr = _make(cuda, graphs=False)
    aug = tr.d_augment
    assert aug.policy == 56 and aug.ada_policy == 56 and aug.diff_policy == 0 and aug.gated and not aug.adaptive
    assert aug.ada_tables.shape == (3, 2, 32) and aug.ctrl.tolist() == [1 << 23] + [0] * 7
    address = aug.ada_tables.data_ptr()
    batches = [_batch(vocab, cuda, 70 + i) for i in range(STEPS)]
    losses, ck2 = [], None
    for n, b in enumerate(batches, 1):
        losses.append(_step(tr, b, n))
        for p in range(3):
            assert np.array_equal(aug.ada_tables[p].cpu().numpy(), ops.ada_pipeline_table_host(0, n, p, 2, 64, 56, 1 << 23).numpy()), (n, p)
        if n == 2:
            ck2 = copy.deepcopy(tr.checkpoint_dict(2, 0))
    assert aug.ada_tables.data_ptr() == address
    return {"vocab": vocab, "batches": batches, "losses": losses, "ck2": ck2, "weights": _weights(tr)}


def test_replayed_equals_eager(cuda, eager_run, monkeypatch):
    """Eager, capture + replay, two replays (the scene-graph encoder's own graph off, as tests/test_gpu_augment.py's
    `encoder_eager`): the ADA stage of passes 0-2 is captured and reads the persistent rows, refilled eagerly before every
    replay.  The policy bits are in the graph key.  Every loss term and every weight, bit for bit."""
    from canonicalsg2im_amd import graphs as csg_graphs
    monkeypatch.setattr(csg_graphs, "MAX_SG_GRAPHS", 0)
    _, tr = _make(cuda, graphs=True)
    assert tr.graphs.key_of(eager_run["batches"][0])[-2:] == (56, "gated")
    got = [_step(tr, b, n) for n, b in enumerate(eager_run["batches"], 1)]
    g = tr.graphs
    assert g.captures == 1 and g.replays == STEPS - 1 and g.eager_steps == 1
    _assert_same_run(got, eager_run["losses"], "replayed against eager")
    _assert_same_weights(_weights(tr), eager_run["weights"], "replayed against eager")


def test_feature_matching_sees_one_transform(cuda):
    """imgs_pred := imgs at p = 1: the generator update's two PatchGAN passes read the same rows (pass 0), so the
    feature-matching distance is exactly 0; rows 0 and 1 give other features; outside a step the input is raw."""
    vocab, tr = _make(cuda, graphs=False, flags=["--d_augment_p", "1"])
    imgs, objs, boxes = _batch(vocab, cuda, 75)[:3]
    tr.discriminator.eval()
    gm, aug = tr.gans_model, tr.d_augment
    with torch.no_grad():
        raw = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
        aug.begin_step()
        try:
            terms = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
            f0 = gm.netD_img(imgs, objs, boxes, aug_pass=0)
            f1 = gm.netD_img(imgs, objs, boxes, aug_pass=1)
        finally:
            aug.end_step()
        after = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
    assert float(terms["GAN_Feat"]) == 0.0, float(terms["GAN_Feat"])
    assert not _same_bits(terms["GAN_Img"], raw["GAN_Img"]), "the augmented pass scored like the raw one"
    assert not _same_bits(f0[0][0], f1[0][0]), "rows 0 and 1 gave the same features"
    assert _same_bits(after["GAN_Img"], raw["GAN_Img"]) and float(raw["GAN_Feat"]) == 0.0


def test_resume(cuda, eager_run):
    """Saved after step 2, loaded into a differently initialised trainer: steps 3 and 4 of the uninterrupted run.  The
    checkpoint carries the names and nothing else new."""
    ck2, batches = eager_run["ck2"], eager_run["batches"]
    assert ck2["d_augment"]["policies"] == ADA and ck2["d_augment"]["iteration"] == 2
    assert set(ck2["d_augment"]) == {"seed", "iteration", "policies", "ctrl", "ada"}
    _, tr = _make(cuda, graphs=False, seed=99)
    assert tr.load_checkpoint(copy.deepcopy(ck2)) == (2, 0) and tr.d_augment.iteration == 2
    got = [_step(tr, batches[n - 1], n) for n in (3, 4)]
    _assert_same_run(got, eager_run["losses"][2:], "resumed against uninterrupted")
    _assert_same_weights(_weights(tr), eager_run["weights"], "resumed against uninterrupted")


def test_p_zero_is_the_raw_run(cuda):
    vocab, off = _make(cuda, graphs=False, policies="", flags=[])
    _, zero = _make(cuda, graphs=False, flags=["--d_augment_p", "0"])
    batch = _batch(vocab, cuda, 91)
    (_, Da), (_, Db) = _step(off, batch, 1), _step(zero, batch, 1)
    assert bool((zero.d_augment.ada_tables[:, :, 13] == ID_FLAGS).all()) and list(Da) == list(Db)
    for k in Da:
        assert _same_bits(Da[k], Db[k]), "%s: %r without --d_augment, %r with p = 0" % (k, float(Da[k]), float(Db[k]))
    _, one = _make(cuda, graphs=False, flags=["--d_augment_p", "1"])
    (_, Dc) = _step(one, batch, 1)
    assert not _same_bits(Da["D_img_real"], Dc["D_img_real"]), "p = 1 scored like no augmentation"


def test_validation_is_raw(cuda):
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, on = _make(cuda, graphs=False, flags=["--d_augment_p", "1"])
    _, off = _make(cuda, graphs=False, policies="", flags=[])
    val = _batch(vocab, cuda, 61)
    a, _, _ = Evaluator(on).check_model([val], use_gt=True)
    b, _, _ = Evaluator(off).check_model([val], use_gt=True)
    assert set(a) == set(b) and on.d_augment.iteration == 0 and not on.d_augment.active
    for k in a:
        assert _same_bits(a[k], b[k]), "%s: %r with the flags, %r without" % (k, float(a[k]), float(b[k]))


@pytest.mark.parametrize("target,start,T24", [("0.6", None, ad.T06), ("0.02", "0.5", 335544)], ids=["target_0.6_from_0", "target_0.02_from_half"])
def test_adaptive_run_moves_p_as_the_host_says(cuda, target, start, T24):
    """K = 2, step24 = 2^23: after every update p24 is the host restatement's `next_p` of the signs counted on the device (read
    back from the record's S_last, C_last and checked against the maps the real pass returned), and the persistent rows are
    the host rows at that p24."""
    from canonicalsg2im_amd import ops
    flags = ["--d_augment_target", target, "--d_augment_interval", "2", "--d_augment_kimg", "0.008"] + (["--d_augment_p", start] if start else [])
    vocab, tr = _make(cuda, graphs=False, flags=flags)
    aug = tr.d_augment
    p24 = int(float(start) * ap.ONE) if start else 0
    assert aug.adaptive and aug.step24 == 1 << 23 and aug.ada["T24"] == T24 and aug.ctrl.tolist() == [p24] + [0] * 7
    seen, inner = [], aug.observe_real

    def observe(scales):
        seen.append([(s[-1] if isinstance(s, (list, tuple)) else s).detach().cpu().numpy() for s in scales])
        return inner(scales)
    aug.observe_real = observe
    moved = []
    for n in range(1, 6):
        _step(tr, _batch(vocab, cuda, 70 + n), n)
        words = aug.ctrl.tolist()
        if n - 1 > 0 and (n - 1) % 2 == 0:                 # begin_step of steps 3 and 5 updated
            counts = [ad.sign_count(m) for m in seen[n - 3:n - 1]]
            S, C = sum(c[0] for c in counts), sum(c[1] for c in counts)
            assert words[4:6] == [S, C], (n, words)
            p24 = ad.next_p(p24, S, C, T24, 1 << 23)
            moved.append(p24)
        print("step %d: words %s" % (n, words))
        assert words[0] == p24, (n, words, p24)
        for p in range(3):
            assert np.array_equal(aug.ada_tables[p].cpu().numpy(), ops.ada_pipeline_table_host(0, n, p, 2, 64, 56, p24).numpy()), (n, p)
    assert len(moved) == 2 and aug.read()["updates"] == 2


def test_both_families_chain_in_the_stated_order(cuda):
    """`color,ada_geom`: the ADA stage first, one launch; DiffAugment's kernel then runs on its output, gated by the same p."""
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.d_augment import DAugment, ada_settings
    aug = DAugment("color,ada_geom", 4, cuda, 3, 16, ada=ada_settings(p=1.0, policies="color,ada_geom"))
    assert (aug.diff_policy, aug.ada_policy) == (1, 16)
    x = _dev(ac.data((3, 16, 8, 0), 77), cuda).permute(0, 3, 1, 2)
    assert aug.apply(x, 1, 4) is x                        # outside a step: raw
    aug.begin_step()
    got = aug.apply(x, 1, 4)
    first = ops.ada_pipeline(x, aug.ada_tables[1], 4)
    want = ops.d_augment(first, aug.tables[1], 4, 1, gate=aug.gates[1])
    other = ops.ada_pipeline(ops.d_augment(x, aug.tables[1], 4, 1, gate=aug.gates[1]), aug.ada_tables[1], 4)
    crops = aug.apply(x, 4, 0)                            # a crop pass: fresh rows of this pass and iteration
    aug.end_step()
    assert _same_bits(got, want) and not _same_bits(got, other) and not _same_bits(got, first)
    assert np.array_equal(aug.ada_tables[1].cpu().numpy(), ops.ada_pipeline_table_host(4, 1, 1, 3, 16, 16, ap.ONE).numpy())
    t4 = _dev(ops.ada_pipeline_table_host(4, 1, 4, 3, 16, 16, ap.ONE).numpy(), cuda)
    g4 = _dev(ops.augment_gate_host(4, 1, 4, 3, ap.ONE).numpy(), cuda)
    assert _same_bits(crops, ops.d_augment(ops.ada_pipeline(x, t4, 0), ops.augment_table(4, 1, 4, 3, 16, device=cuda), 0, 1, gate=g4))
    with pytest.raises(ValueError, match="need the strength settings"):
        DAugment("ada_blit", 0, cuda, 2, 16)
