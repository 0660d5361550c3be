"""Every launch rule of the direct convolution (csrc/igemm.hip) through the C ABI - csg_conv_fwd, csg_conv_fwd_multi,
csg_conv_bwd_weight as `_lib` binds them - and `ops.conv2d_forward` on a real MI355X, against the float64 restatement of the
contract (tests/igemm_cases.py: the table, `desc_ref64`, `wgrad_ref64`).

Per row: the allocator's free blocks are filled with NaN before each run, so a slab, an output row or a gradient no kernel
writes shows up as NaN; every output must be finite, a second run must reproduce it bit for bit (slabs are summed in a
fixed order), and every entry of y the descriptor does not own - the channels before and after a slice, the other parity
classes' pixels - must keep the value it held, bit for bit.  A row that accumulates starts from seeded non-zero values in y
and the reference adds them.  A multi row must also equal its four classes launched one by one (bit for bit where both
take the same split).

Gates.  Forward outputs: max error <= 1e-5 of the fp64 tensor's largest entry plus a 1e-6 floor (test_gpu_conv_plans.GATE /
FLOOR).  dw and db add up to 66 564 terms, so no fixed fraction can be derived for them: they are held against the float32
CPU evaluation of the same restatement on the same inputs, hip_err <= max(3 x fp32_cpu_err, 1e-5 x scale) + 1e-6 (the band
of the other matrices).  No row masks, drops or loosens anything: the outputs are continuous in the inputs, and res_gate
reads the sign of given data.  The measured pairs of every row are in profiles/igemm_paths_gpu.txt."""
import ctypes
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

import igemm_cases as ic
from igemm_cases import CASES, ENTRY_CASES, case_ids
from test_gpu_conv_plans import FLOOR, GATE, _nan_fill

pytestmark = pytest.mark.gpu
BAND = 3.0
REPORT = os.environ.get("IGEMM_PATHS_REPORT")         # a file that receives the table too (profiles/igemm_paths_gpu.txt)

HEADER = """tests/test_gpu_igemm_paths.py on an MI355X (gfx950): one line per row and tensor - the launch class the restated rules give
the row (bn, m-tiles x n-tiles, K tiles, plain | ksplit | tail(first split tile, slabs, first slab row), set | acc, vec |
scalar epilogue; bi, i-tiles x j-tiles, nsplit, chunks per split for a weight gradient), the largest fp64 entry (scale), the
HIP error and the float32 CPU restatement's error on the same inputs, both as fractions of the scale, and the rule the tensor
is held to: gate = 1e-5 of the scale + 1e-6; band = max(3 x fp32 error, 1e-5 of the scale) + 1e-6 (dw, db).  Written by the
test itself when IGEMM_PATHS_REPORT names a file.
"""
_report = []          # the open report file, once per session


def _say(line, report=True):
    print(line, file=sys.stderr)
    if REPORT and report:
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


def _workspace(nbytes, what):
    assert nbytes >= 0, what
    return torch.empty(nbytes // 4, device="cuda", dtype=torch.float32) if nbytes else None


def _forward(L, row, data, singly=False):
    """y after the row's launch (for a multi row with `singly`: its classes through csg_conv_fwd one by one)."""
    x, w, bias, res, y = (_dev(data[k]) for k in ("x", "w", "bias", "res", "y0"))
    xo, yo = row["x_off"], row["y_off"]
    if row["entry"] == "multi" and not singly:
        arr, n = ic.desc_array(row["descs"]), len(row["descs"])
        nbytes = L.lib.csg_conv_fwd_multi_workspace(arr, n)
        if row["refuse"]:                                              # the query refuses already (-1): the launch must as well
            nbytes = max(nbytes, 0)
        ws = _workspace(nbytes, row["name"])
        L.check(L.lib.csg_conv_fwd_multi(arr, n, _p(x, xo), _p(w), _p(bias), _p(res, yo), _p(y, yo), _p(ws), nbytes, L.stream()), row["name"])
    else:
        for d in row["descs"]:
            cd = ic.to_ctypes(d)
            nbytes = L.lib.csg_conv_fwd_workspace(cd)
            ws = _workspace(nbytes, row["name"])
            given = nbytes - 4 if row["short_ws"] else nbytes
            L.check(L.lib.csg_conv_fwd(cd, _p(x, xo), _p(w), _p(bias), _p(res, yo), _p(y, yo), _p(ws), given, L.stream()), row["name"])
    torch.cuda.synchronize()
    return dict(y=y.cpu())


def _wgrad(L, row, data):
    (d,) = row["descs"]
    cd = ic.to_ctypes(d)
    x, dy = _dev(data["x"]), _dev(data["dy"])
    dw = torch.full(ic.buffers(row)["dw"], float("nan"), device="cuda")
    db = torch.full((d["Cout"],), float("nan"), device="cuda") if row["db"] else None
    nbytes = L.lib.csg_conv_bwd_weight_workspace(cd)
    ws = _workspace(nbytes, row["name"])
    L.check(L.lib.csg_conv_bwd_weight(cd, _p(x, row["x_off"]), _p(dy, row["y_off"]), _p(dw), _p(db), _p(ws), nbytes, L.stream()), row["name"])
    torch.cuda.synchronize()
    return dict(dw=dw.cpu(), db=None if db is None else db.cpu())


def _run(L, row, data):
    return _wgrad(L, row, data) if row["entry"] == "wgrad" else _forward(L, row, data)


def _judge(row, name, got, ref, fp32, rule, own=None):
    """None, or what is wrong with tensor `name`; `own`: the entries the launch owns (the rest is compared bit for bit by
    the caller)."""
    assert tuple(got.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (row["name"], name, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote?)" % (row["name"], name, bad)
    if own is not None:
        g, ref, fp32 = g[own], ref[own], fp32[own]
    scale = float(ref.abs().max())
    err = float((g - ref).abs().max())
    ferr = float((fp32.double() - ref).abs().max())
    allow = (GATE * scale if rule == "gate" else max(BAND * ferr, GATE * scale)) + FLOOR
    _say("| %-26s | %-2s | %-64s | scale %.2e | hip %.2e | fp32 %.2e | %s |" % (
        row["name"], name, ic.describe(row)[:64], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300), rule))
    return None if err <= allow else "%s %s: max error %.3e, allowed %.3e (scale %.3e, fp32 error %.3e, %s)" % (
        row["name"], name, err, allow, scale, ferr, rule)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _refuse(L, row, data):
    with pytest.raises(RuntimeError, match=row["refuse"]):
        _run(L, row, data)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_launch_rule_against_fp64(L, c):
    t0 = time.time()
    data = ic.make_data(c)
    if c["refuse"]:
        _refuse(L, c, data)
        return
    runs = []
    for _ in range(2):
        _nan_fill()
        runs.append(_run(L, c, data))
    ref, fp32 = ic.reference(c, data), ic.reference(c, data, torch.float32)
    failures = []
    if c["kind"] == "wgrad":
        for name in ("dw", "db"):
            if ref[name] is None:
                assert runs[0][name] is None
                continue
            msg = _judge(c, name, runs[0][name], ref[name], fp32[name], "band")
            if msg:
                failures.append(msg)
            assert _same_bits(runs[0][name], runs[1][name]), "%s %s: a second run differs" % (c["name"], name)
    else:
        y, own = runs[0]["y"], ref["own"]
        msg = _judge(c, "y", y, ref["y"], fp32["y"], "gate", own)
        if msg:
            failures.append(msg)
        assert _same_bits(y, runs[1]["y"]), "%s: a second run differs" % c["name"]
        assert _same_bits(y[~own], data["y0"][~own]), "%s: %d entries outside the launch's slice changed" % (
            c["name"], int((y[~own].view(torch.int32) != data["y0"][~own].view(torch.int32)).sum()))
        assert bool(own.any()) and (c["y_off"] == 0 or bool((~own).any())), c["name"]
        if c["kind"] == "multi":
            _nan_fill()
            one = _forward(L, c, data, singly=True)["y"]
            same_split = [p["ksplit"] for p in ic.multi_plan(c["descs"])[0]] == [ic.fwd_plan(d)["ksplit"] for d in c["descs"]]
            if same_split:
                assert _same_bits(y, one), "%s: one launch differs from the four single launches" % c["name"]
            else:
                scale = float(ref["y"].abs().max())
                assert float((y.double() - one.double()).abs().max()) <= GATE * scale + FLOOR, c["name"]
    _say("| %-26s | time | %.2f s |" % (c["name"], time.time() - t0), report=False)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("e", ENTRY_CASES, ids=[e["name"] for e in ENTRY_CASES])
def test_python_entry_against_fp64(L, e):
    """ops.conv2d_forward with bias and ReLU into channels [off, off + Cout) of a wider map: the 5x5 layer with 64 input
    channels (two launches, both split along K, the second accumulates, csg_bias_act on the sum) and the (1,7) layer at the
    batch that tail-splits.  The reference is torch's own float64 convolution."""
    from canonicalsg2im_amd import ops
    t0 = time.time()
    g = torch.Generator().manual_seed(len(e["name"]))
    x = torch.randn(e["B"], e["Cin"], e["H"], e["W"], generator=g)
    w = torch.randn(e["Cout"], e["Cin"], e["KH"], e["KW"], generator=g) * (2.0 / (e["Cin"] * e["KH"] * e["KW"])) ** 0.5
    b = 0.3 * torch.randn(e["Cout"], generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), 1, e["pad"]))
    fp32 = F.relu(F.conv2d(x, w, b, 1, e["pad"]))
    runs = []
    for _ in range(2):
        _nan_fill()
        wide = ops.nhwc(torch.full((e["B"], e["wide"], e["H"], e["W"]), ic.SENTINEL, device="cuda"))
        with torch.no_grad():
            ops.conv2d_forward(ops.nhwc(x.cuda()), w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(), e["KH"], e["KW"], 1, e["pad"],
                               ops.ACT_LEAKY, 0.0, out=wide, out_off=e["off"])
        torch.cuda.synchronize()
        runs.append(wide.cpu())
    got = runs[0]
    lo, hi = e["off"], e["off"] + e["Cout"]
    assert bool((got[:, :lo] == ic.SENTINEL).all()) and bool((got[:, hi:] == ic.SENTINEL).all()), "%s: the slice's neighbours changed" % e["name"]
    row = dict(name=e["name"], kind="fwd", entry="fwd", descs=ic.entry_descs(e), db=False)
    msg = _judge(row, "y", got[:, lo:hi], ref, fp32, "gate")
    assert _same_bits(got, runs[1]), "%s: a second run differs" % e["name"]
    _say("| %-26s | time | %.2f s |" % (e["name"], time.time() - t0), report=False)
    assert msg is None, msg
