"""Every launch rule of the Winograd kernels (csrc/wino.hip, wino4.hip, wino4w.hip; host side csrc/csg_wino_host.h) through
the C ABI - the pack, convolution, conv_part / conv_spade and weight-gradient entry points as `_lib` binds them - on a real
MI355X, against the float64 restatement of the contract (tests/wino_cases.py: the table, `wino_ref64`, `wino_wgrad_ref64`).

Per row: the allocator's free blocks are filled with NaN before each run, the packed operand, the slabs of a split and the
gradients start as NaN, and every channel of an input outside the slice the kernel may read holds NaN - a lane, slab, output
or gradient no kernel writes, or a read past a slice, shows up as NaN; every output must be finite, a second run must
reproduce it bit for bit (slabs are summed in a fixed order), and every entry of y (and gamma_out) the descriptor does not
own must keep its sentinel, bit for bit.  A pack from a strided weight must equal the pack of its contiguous copy bit for
bit.  A row whose workspace is 4 bytes short must equal the NULL-workspace run bit for bit; a persistent row runs with
csg_wino4_persistent(1) and (0) and the two must agree bit for bit; a csg_wino4_conv_spade row must equal the
csg_wino4_conv_part pair bit for bit.  A refusal row must return its documented code and leave every output untouched.

Gate for y, gamma_out, dw and db: max error <= 1e-5 of the fp64 tensor's largest entry plus a 1e-6 floor
(test_gpu_conv_plans.GATE / FLOOR: the acceptance gate of these kernels, tests/test_gpu_wino4.py, held there at far longer
sums).  No row masks or drops entries: the epilogues are continuous, and the gate reads the sign of given data.  The
table the test writes when WINO_PATHS_REPORT names a file has one line per row and tensor.  The convolution entries take a
dense x only (refusal rows); strided x is run by the weight-gradient rows."""
import ctypes
import os
import re
import sys
import time

import pytest
import torch

import wino_cases as wc
from test_gpu_conv_plans import FLOOR, GATE, _nan_fill
from wino_cases import CASES, PACK_TAILS, case_ids

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("WINO_PATHS_REPORT")          # a file that receives the table too
RUN = [c for c in CASES if not c["refuse"]]
REFUSE = [c for c in CASES if c["refuse"]]
NAN = float("nan")

HEADER = """tests/test_gpu_wino_paths.py on an MI355X (gfx950): one line per row and tensor - the launch class the restated rules give
the row (family and instantiation, blocks, stages, plain | split ksplit sps | unsplit-*, epilogue; for a weight gradient
cout-blocks x cin-blocks, regions, slices, regions per slice), the largest fp64 entry (scale), the HIP error and the float32
CPU restatement's error on the same inputs, both as fractions of the scale, and the seconds the row took (both runs, the
references and every comparison).  Every tensor is held to 1e-5 of the scale + 1e-6.  Written by the test itself when
WINO_PATHS_REPORT names a file.
"""
_report = []          # the open report file, once per session


def _say(line):
    print(line, file=sys.stderr)
    if REPORT:
        if not _report:
            _report.append(open(REPORT, "w"))
            _report[0].write(HEADER + "\n")
        _report[0].write(line + "\n")
        _report[0].flush()


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import _lib
    return _lib


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def _dev(t):
    return None if t is None else t.to(torch.float32).cuda()


def _nans(n):
    return torch.full((max(int(n), 1),), NAN, device="cuda")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ packs
def _pack_fn(L, fam):
    return {"f2": (L.lib.csg_wino_pack_weights, L.lib.csg_wino_pack_bytes), "f4": (L.lib.csg_wino4_pack_weights, L.lib.csg_wino4_pack_bytes),
            "f34": (L.lib.csg_wino34_pack_weights, L.lib.csg_wino4_pack_bytes)}[fam]


def _place_weight(w, fmt):
    """The (O, I, k, k) weight on the device: contiguous, channels-last, or a channel slice of a larger parameter whose
    other entries are NaN."""
    w = w.cuda()
    if fmt == "cl":
        return w.contiguous(memory_format=torch.channels_last)
    if fmt == "slice":
        big = torch.full((w.shape[0] + 8, w.shape[1] + 12) + tuple(w.shape[2:]), NAN, device="cuda")
        big[4:4 + w.shape[0], 8:8 + w.shape[1]] = w
        return big[4:4 + w.shape[0], 8:8 + w.shape[1]]
    return w.contiguous()


def _pack_one(L, fam, w, bwd, sigma, what):
    O, I = w.shape[:2]
    N, K = (I, O) if bwd else (O, I)
    fn, nbytes = _pack_fn(L, fam)
    n = nbytes(N, K)
    assert n == wc.wino_pack_bytes(wc.POSITIONS[fam], N, K) > 0, what
    packed = _nans(n // 4)
    L.check(fn(_p(w), *w.stride(), O, I, int(bwd), _p(sigma), _p(packed), L.stream()), what)
    torch.cuda.synchronize()
    bad = int((~torch.isfinite(packed)).sum())
    assert bad == 0, "%s: %d lanes of the packed operand were not written" % (what, bad)
    return packed


def _pack(L, row, data):
    """The row's packed operand; a strided weight's pack must be the pack of its contiguous copy."""
    w, sigma = _place_weight(data["w"], row["wfmt"]), _dev(data["sigma"])
    packed = _pack_one(L, row["fam"], w, row["bwd"], sigma, row["name"] + " pack")
    if row["wfmt"] != "contig":
        assert not w.is_contiguous()
        twin = _pack_one(L, row["fam"], w.contiguous(), row["bwd"], sigma, row["name"] + " pack (contiguous copy)")
        assert _same_bits(packed, twin), "%s: the pack of the %s weight differs from its contiguous copy's" % (row["name"], row["wfmt"])
    return packed


@pytest.mark.parametrize("fam,O,I", PACK_TAILS, ids=["%s_%dx%d" % t for t in PACK_TAILS])
def test_pack_zeroes_the_padded_lanes(L, fam, O, I):
    """K no multiple of 8 and N no multiple of 32: the lanes past the weight are zero - the pack equals, bit for bit, the pack
    of the weight padded with zeros to whole 32 x 8 blocks - in both operand orders, from a NaN-filled buffer."""
    k = 4 if fam == "f34" else 3
    g = torch.Generator().manual_seed(O * 100 + I)
    w = torch.randn(O, I, k, k, generator=g).cuda()
    Op, Ip = wc.cdiv(O, 32) * 32, wc.cdiv(I, 32) * 32
    wide = torch.zeros(Op, Ip, k, k, device="cuda")
    wide[:O, :I] = w
    for bwd in (False, True):
        a = _pack_one(L, fam, w, bwd, None, "tail pack")
        b = _pack_one(L, fam, wide, bwd, None, "padded pack")
        Na, Ka = (I, O) if bwd else (O, I)
        # same NT32; the padded weight has more k-octets per (position, tile): compare the octets the narrow one has
        pos, nt, qa, qb = wc.POSITIONS[fam], wc.cdiv(Na, 32), wc.cdiv(Ka, 8), (Op if bwd else Ip) // 8
        assert _same_bits(a.view(pos * nt, qa, 256), b.view(pos * nt, qb, 256)[:, :qa].contiguous()), (fam, O, I, bwd)
        assert bool((b.view(pos * nt, qb, 256)[:, qa:] == 0).all())


# ------------------------------------------------------------------------------------------------ launches
def _conv_call(L, row, dv, packed, y, ws, nbytes):
    cd, fam = wc.to_ctypes(row["d"]), row["fam"]
    xo, yo = row["x_off"], row["y_off"]
    args = (_p(dv["x"], xo), _p(packed), _p(dv["bias"]), _p(dv["res"], yo), _p(dv["gate"], yo), row["gate_slope"], _p(y, yo), _p(ws), nbytes,
            L.stream())
    if fam == "f2":
        return L.lib.csg_wino_conv(cd, *args)
    if fam == "f4":
        return L.lib.csg_wino4_conv(cd, *args)
    return L.lib.csg_wino34_conv(cd, row["pad"], *args)


def _workspace_query(L, row):
    cd = wc.to_ctypes(row["d"])
    return {"f2": lambda: L.lib.csg_wino_conv_workspace(cd), "f4": lambda: L.lib.csg_wino4_conv_workspace(cd),
            "f34": lambda: L.lib.csg_wino34_conv_workspace(cd, row["pad"])}[row["fam"]]()


def _part_call(L, row, dv, packed, y, part, d=None, y_off=None, bias_off=None):
    cd = wc.to_ctypes(row["d"] if d is None else d)
    yo = row["y_off"] if y_off is None else y_off
    t0 = 32 * part["tile_off"] if bias_off is None else bias_off
    if part["mod"]:
        mod = (_p(dv["mod_x"], row["y_off"]), _p(dv["mod_gamma"], part["g_off"]), part["gamma_cs"], _p(dv["mean"]), _p(dv["invstd"]), part["mod_slope"])
    else:
        mod = (None, None, 0, None, None, 1.0)
    return L.lib.csg_wino4_conv_part(cd, _p(dv["x"], row["x_off"]), _p(packed), part["tile_off"], part["tiles_total"], _p(dv["bias"], t0),
                                     *mod, _p(y, yo), L.stream())


def _forward(L, row, data, ws_mode=None):
    """{y[, gamma_out]} after the row's launch, on the CPU.  ws_mode: given | short | null (default: the row's)."""
    dv = {k: _dev(v) for k, v in data.items() if torch.is_tensor(v) or v is None}
    packed = _pack(L, row, data)
    y = dv["y0"].clone()
    out = {}
    if row["entry"] == "part":
        L.check(_part_call(L, row, dv, packed, y, row["part"]), row["name"])
    elif row["entry"] == "spade":
        sp = row["spade"]
        gout = dv["gamma0"].clone() if sp["gamma_out"] else None
        cd = wc.to_ctypes(row["d"])
        assert L.lib.csg_wino4_conv_spade_supported(cd) == 1, "%s: the launch does not qualify on this device (%d CUs)" % (
            row["name"], torch.cuda.get_device_properties(0).multi_processor_count)
        L.check(L.lib.csg_wino4_conv_spade(cd, _p(dv["x"], row["x_off"]), _p(packed), _p(dv["bias"]), _p(dv["mod_x"], row["y_off"]),
                                           _p(gout, sp["g_off"]), sp["gamma_cs"], _p(dv["mean"]), _p(dv["invstd"]), sp["mod_slope"],
                                           _p(y, row["y_off"]), L.stream()), row["name"])
        if gout is not None:
            out["gamma_out"] = gout
    else:
        mode = row["ws"] if ws_mode is None else ws_mode
        nbytes = _workspace_query(L, row)
        plan, kind = wc.run_plan(row)
        assert nbytes == wc.conv_workspace_bytes(row["fam"], row["d"], row["pad"]) >= 0, row["name"]
        ws, given = None, 0
        if mode == "given" and nbytes:
            ws, given = _nans(nbytes // 4), nbytes                     # a split row's slabs start as NaN
        elif mode == "short":
            assert nbytes >= 8, row["name"]
            ws, given = _nans(nbytes // 4 - 1), nbytes - 4             # a real buffer, one float too small
        L.check(_conv_call(L, row, dv, packed, y, ws, given), row["name"])
    torch.cuda.synchronize()
    out["y"] = y
    return {k: v.cpu() for k, v in out.items()}


def _spade_as_part_pair(L, row, data):
    """The same SPADE modulation as two csg_wino4_conv_part launches: gamma into a (B, H, W, gamma_cs) map, then the beta half."""
    dv = {k: _dev(v) for k, v in data.items() if torch.is_tensor(v) or v is None}
    packed = _pack(L, row, data)
    sp, d = row["spade"], row["d"]
    tiles = d["Cout"] // 32
    gbuf = dv["gamma0"].clone()
    L.check(_part_call(L, row, dv, packed, gbuf, dict(tile_off=0, tiles_total=2 * tiles, mod=False), d=dict(d, y_cs=sp["gamma_cs"]),
                       y_off=sp["g_off"]), row["name"] + " gamma half")
    y = dv["y0"].clone()
    dv["mod_gamma"] = gbuf
    L.check(_part_call(L, row, dv, packed, y, dict(tile_off=tiles, tiles_total=2 * tiles, mod=True, gamma_cs=sp["gamma_cs"], g_off=sp["g_off"],
                                                   mod_slope=sp["mod_slope"])), row["name"] + " beta half")
    torch.cuda.synchronize()
    return dict(y=y.cpu(), gamma_out=gbuf.cpu())


def _wg_fns(L, fam):
    return ((L.lib.csg_wino_bwd_weight, L.lib.csg_wino_bwd_weight_workspace) if fam == "wg2" else
            (L.lib.csg_wino4_bwd_weight, L.lib.csg_wino4_bwd_weight_workspace))


def _wgrad(L, row, data, short=False):
    d = row["d"]
    cd = wc.to_ctypes(d)
    fn, query = _wg_fns(L, row["fam"])
    x, dy = _dev(data["x"]), _dev(data["dy"])
    dw = torch.full((d["Cout"], 3, 3, d["Cin"]), NAN, device="cuda")
    db = torch.full((d["Cout"],), NAN, device="cuda") if row["db"] else None
    nbytes = query(cd)
    assert nbytes == wc.wg_workspace_bytes(row["fam"], d) > 0, row["name"]
    slabs = wc.wg_plan(row["fam"], d)["nslab"] * d["Cout"] * 9 * d["Cin"]
    ws = _nans(nbytes // 4)
    rc = fn(cd, _p(x, row["x_off"]), _p(dy, row["y_off"]), _p(dw), _p(db), _p(ws), nbytes - 4 if short else nbytes, L.stream())
    torch.cuda.synchronize()
    if not row["db"]:                                                  # with db = NULL the db rows behind the dW slabs take no part
        assert bool(torch.isnan(ws[slabs:]).all()), "%s: db slab rows were written although db is NULL" % row["name"]
    return rc, dict(dw=dw.cpu(), db=None if db is None else db.cpu())


def _run(L, row, data):
    if row["entry"] == "wgrad":
        rc, out = _wgrad(L, row, data)
        L.check(rc, row["name"])
        return out
    return _forward(L, row, data)


def _judge(row, name, got, ref, fp32, own=None):
    """(line for the report, None or what is wrong with tensor `name`); `own`: the entries the launch owns (the rest is
    compared bit for bit by the caller)."""
    assert tuple(got.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (row["name"], name, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote, or a read outside the slice)" % (row["name"], name, bad)
    if own is not None:
        g, ref, fp32 = g[own], ref[own], fp32[own]
    scale = float(ref.abs().max())
    err = float((g - ref).abs().max())
    ferr = float((fp32.double() - ref).abs().max())
    allow = GATE * scale + FLOOR
    line = "| %-36s | %-9s | %-72s | scale %.2e | hip %.2e | fp32 %.2e |" % (
        row["name"], name, wc.describe(row)[:72], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300))
    return line, None if err <= allow else "%s %s: max error %.3e, allowed %.3e (scale %.3e, fp32 error %.3e)" % (
        row["name"], name, err, allow, scale, ferr)


def _both_forms(L, fn):
    """fn() with the persistent form of k_wino4_conv_v switched on, then off; the previous setting is put back (an undecided
    one, -1, cannot be set again: then what CSG_WINO4_PERSIST would have decided, default on)."""
    prev = L.lib.csg_wino4_persistent(1)
    try:
        on = fn()
        L.lib.csg_wino4_persistent(0)
        off = fn()
    finally:
        L.lib.csg_wino4_persistent(prev if prev >= 0 else int(int(os.environ.get("CSG_WINO4_PERSIST", "1")) != 0))
    return on, off


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_launch_rule_against_fp64(L, c):
    t0 = time.time()
    data = wc.buffers(c)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if c["both_forms"] or c["entry"] == "spade":
        assert ("f4", "form", "persistent") in wc.classify(c, cus), "%s: not a persistent launch on %d CUs" % (c["name"], cus)
    runs = []
    for _ in range(2):
        _nan_fill()
        runs.append(_run(L, c, data))
    ref, fp32 = wc.reference(c, data), wc.reference(c, data, torch.float32)
    lines, failures = [], []
    if c["entry"] == "wgrad":
        for name in ("dw", "db"):
            if ref[name] is None:
                assert runs[0][name] is None
                continue
            line, msg = _judge(c, name, runs[0][name], ref[name], fp32[name])
            lines.append(line)
            failures += [msg] if msg else []
            assert _same_bits(runs[0][name], runs[1][name]), "%s %s: a second run differs" % (c["name"], name)
    else:
        for name, own, start in (("y", "own", "y0"), ("gamma_out", "gamma_own", "gamma0")):
            if name not in ref:
                assert name not in runs[0]
                continue
            got, mask = runs[0][name], ref[own]
            line, msg = _judge(c, name, got, ref[name], fp32[name], mask)
            lines.append(line)
            failures += [msg] if msg else []
            assert _same_bits(got, runs[1][name]), "%s %s: a second run differs" % (c["name"], name)
            assert _same_bits(got[~mask], data[start][~mask]), "%s %s: %d entries outside the launch's slice changed" % (
                c["name"], name, int((got[~mask].view(torch.int32) != data[start][~mask].view(torch.int32)).sum()))
            assert bool(mask.any()) and (c["y_off"] == 0 or bool((~mask).any())), c["name"]
        if c["ws"] == "short":                                         # too small by one float: exactly the NULL-workspace launch
            _nan_fill()
            assert _same_bits(runs[0]["y"], _forward(L, c, data, "null")["y"]), "%s: differs from the NULL-workspace run" % c["name"]
            _nan_fill()
            split = _forward(L, c, data, "given")["y"]                 # and the split launch it declined is a different sum, equally right
            assert float((split.double() - ref["y"]).abs().max()) <= GATE * float(ref["y"].abs().max()) + FLOOR, c["name"]
        if c["both_forms"]:
            _nan_fill()
            on, off = _both_forms(L, lambda: _forward(L, c, data)["y"])
            assert _same_bits(on, off), "%s: the persistent and the one-item form differ" % c["name"]
            assert _same_bits(on, runs[0]["y"]), c["name"]
        if c["entry"] == "spade":
            _nan_fill()
            pair = _spade_as_part_pair(L, c, data)
            assert _same_bits(runs[0]["y"], pair["y"]), "%s: y differs from the csg_wino4_conv_part pair" % c["name"]
            if c["spade"]["gamma_out"]:
                assert _same_bits(runs[0]["gamma_out"], pair["gamma_out"]), "%s: gamma_out differs from the pair's gamma map" % c["name"]
    for line in lines:
        _say("%s %.2f s |" % (line, time.time() - t0))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("c", REFUSE, ids=case_ids(REFUSE))
def test_refusals_launch_nothing(L, c):
    """The documented code, and every output still holds what it held."""
    code, text = c["refuse"]
    row = wc.safe_row(c)
    data = wc.buffers(row)
    _nan_fill()
    if c["entry"] == "wgrad":
        rc, out = _wgrad(L, row, data, short=True)
        assert rc == code and text in L.last_error(), (rc, L.last_error())
        assert bool(torch.isnan(out["dw"]).all()) and (out["db"] is None or bool(torch.isnan(out["db"]).all()))
        return
    dv = {k: _dev(v) for k, v in data.items() if torch.is_tensor(v) or v is None}
    how = c["how"]
    if how == "pack":
        fn, nbytes = _pack_fn(L, c["fam"])
        w = dv["w"]
        packed = _nans(nbytes(w.shape[0], w.shape[1]) // 4 + 4)
        rc = fn(_p(w), *w.stride(), w.shape[0], w.shape[1], 0, None, _p(packed, 1), L.stream())
        torch.cuda.synchronize()
        assert rc == code and text in L.last_error(), (rc, L.last_error())
        assert bool(torch.isnan(packed).all())
        return
    packed = _pack(L, row, data)
    packed = torch.cat([packed, packed[:4]])                           # room for the pointer that is 4 bytes off
    y = torch.cat([dv["y0"].flatten(), dv["y0"].flatten()[:4]])
    x = torch.cat([dv["x"].flatten(), dv["x"].flatten()[:4]])
    cd = wc.to_ctypes(c["d"])                                          # the refused descriptor itself
    px, pp, py = _p(x, int(how == "x")), _p(packed, int(how == "packed")), _p(y, int(how == "y"))
    if c["entry"] == "part":
        pt = c["part"]
        rc = L.lib.csg_wino4_conv_part(cd, px, pp, pt["tile_off"], pt["tiles_total"], _p(dv["bias"]), None, None, 0, None, None, 1.0, py, L.stream())
    elif c["entry"] == "spade":
        assert L.lib.csg_wino4_conv_spade_supported(cd) == 0
        rc = L.lib.csg_wino4_conv_spade(cd, px, pp, _p(dv["bias"]), _p(dv["mod_x"]), None, 0, _p(dv["mean"]), _p(dv["invstd"]), 0.2, py, L.stream())
    elif c["fam"] == "f34":
        rc = L.lib.csg_wino34_conv(cd, c["pad"], px, pp, None, None, None, 0.0, py, None, 0, L.stream())
    else:
        fn = L.lib.csg_wino_conv if c["fam"] == "f2" else L.lib.csg_wino4_conv
        rc = fn(cd, px, pp, None, None, None, 0.0, py, None, 0, L.stream())
    torch.cuda.synchronize()
    assert rc == code, (c["name"], rc, L.last_error())
    assert re.search(text, L.last_error()), (c["name"], L.last_error())
    assert bool((y == wc.SENTINEL).all()), "%s: a refused call wrote to y" % c["name"]
