"""Every launch rule of the plain GEMMs (csrc/gemm.hip) and of the few-output convolutions (csrc/fewn.hip) through the C ABI -
csg_gemm_nt, csg_gemm_tn, csg_conv_few_fwd / _bwd_data / _bwd_weight as `_lib` binds them - and two rows through `ops` on a
real MI355X, against the float64 restatement of the contract (tests/gemm_few_cases.py: the table, the references, the data).

Per row and data kind: the allocator's free blocks are filled with NaN before each run, and so is every workspace; the pad
columns of every input row stride, channels [Cin, x_cs) of x and the weight rows and bias entries beyond cout_real hold NaN;
outputs start as NaN where the launch owns them and as a sentinel where it does not.  Every owned output must be finite,
every other entry must keep its bits (y's columns [N, ldy), dx's channels [Cin, x_cs), the workspace of a direct tn launch
and of a forward that was handed too little), and a second run must reproduce every output bit for bit.  Few-output rows
carry 0.75 in dy's pad channels; y, dw and db must hold exact zeros beyond cout_real.

"exact" data (small integers, power-of-two slopes): the output must EQUAL the float64 reference.  "random" data: hip_err <=
max(3 x fp32_cpu_err, 1e-5 x scale) + 1e-6 with the float32 CPU evaluation of the same restatement on the same inputs -
GATE, FLOOR and BAND of test_gpu_igemm_paths.py, imported, not chosen here.  Nothing is masked or dropped: every output is
continuous in the inputs, the gates read the sign of given data, and the entry row's hidden layer keeps clear of the ReLU's
kink by construction (gemm_few_cases.entry_data).  The measured pairs of every row are in profiles/gemm_few_paths_gpu.txt."""
import ctypes
import os
import sys
import time

import pytest
import torch

import gemm_few_cases as gc
from gemm_few_cases import CASES, ENTRY_CASES, KINDS, REFUSALS, SENTINEL
from test_gpu_conv_plans import _nan_fill
from test_gpu_igemm_paths import BAND, FLOOR, GATE

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("GEMM_FEW_PATHS_REPORT")     # a file that receives the table too (profiles/gemm_few_paths_gpu.txt)
NAN = float("nan")

HEADER = """tests/test_gpu_gemm_few_paths.py on an MI355X (gfx950): one line per row, data kind and tensor - the numbers the restated
launch rules give the row (nt: tile, BK, stages, 16-byte slots of a K tail, grid; tn: direct | narrow | wide slab sum, slices,
rows per slice, rows of the last; few: forward TX, tiles, chunks per split, ksplit and how the channels are cut | backward
pixel lanes PL, pixels per block, blocks, pixels of the last block, output pixels per block for db), the largest fp64 entry
(scale), the HIP error and the float32 CPU restatement's error on the same inputs, both as fractions of the scale, and the
rule: band = max(3 x fp32 error, 1e-5 of the scale) + 1e-6 for random data, equal = no tolerance for exact (integer) data.
Written by the test itself when GEMM_FEW_PATHS_REPORT names a file.
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


@pytest.fixture()
def gemm_ops():
    """`ops` with every shape on the GEMM kernels, however few tiles it has; restored afterwards."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops
    old = ops.GEMM_MODE, ops.GEMM_MIN_TILES
    ops.GEMM_MODE, ops.GEMM_MIN_TILES = "all", 1
    yield ops
    ops.GEMM_MODE, ops.GEMM_MIN_TILES = old


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(t):
    return None if t is None else t.to(torch.float32).cuda()


def _filled(shape, value):
    n = int(torch.Size(shape).numel())
    return torch.full(shape, value, device="cuda", dtype=torch.float32) if n else None


def _owned(shape, width, cols):
    """A NaN output of `shape` whose trailing axis belongs to the launch in [0, cols) only: the sentinel beyond."""
    t = torch.full(shape, NAN, device="cuda", dtype=torch.float32)
    if cols < width:
        t[..., cols:] = SENTINEL
    return t


def _run_nt(L, r, data):
    a, bw, bias, gate = (_dev(data[k]) for k in ("a", "bw", "bias", "gate"))
    y = _owned((r["M"], r["ldy"]), r["ldy"], r["N"])
    L.check(L.lib.csg_gemm_nt(gc.nt_to_ctypes(r), _p(a), _p(bw), _p(bias), _p(gate), _p(y), L.stream()), r["name"])
    torch.cuda.synchronize()
    return dict(y=y.cpu())


def _run_tn(L, r, data):
    M, N, K = r["M"], r["N"], r["K"]
    dy, x = _dev(data["dy"]), _dev(data["x"])
    dw, db = _filled((N, K), NAN), (_filled((N,), NAN) if r["db"] else None)
    nbytes = L.lib.csg_gemm_tn_workspace(M, N, K)
    assert nbytes == gc.tn_plan(M, N, K)["ws_bytes"], r["name"]
    # a direct launch is handed a workspace all the same: it must not touch it
    ws = _filled((nbytes // 4,), NAN) if nbytes else _filled((256,), SENTINEL)
    given = nbytes or 1024
    L.check(L.lib.csg_gemm_tn(M, N, K, _p(dy), r["ldy"], _p(x), r["ldx"], _p(dw), _p(db), _p(ws), given, L.stream()), r["name"])
    torch.cuda.synchronize()
    return dict(dw=dw.cpu(), db=None if db is None else db.cpu(), ws_kept=None if nbytes else ws.cpu())


def _run_few(L, r, data):
    d = r["desc"]
    cd, s, out = gc.few_to_ctypes(d), gc.buffers(r), {}
    x, w, bias, dy = (_dev(data[k]) for k in ("x", "w", "bias", "dy"))
    if "fwd" in r["dirs"]:
        y = _filled(s["y"], NAN)
        nbytes = L.lib.csg_conv_few_fwd_workspace(cd)
        assert nbytes == gc.few_fwd_plan(d)["ws_bytes"], r["name"]
        if r["ws"] == "full":
            ws, given = _filled(s["ws_fwd"], NAN), nbytes
        elif r["ws"] == "none":
            ws, given = None, 0
        else:
            ws, given = _filled(s["ws_fwd"], SENTINEL), nbytes - 4
        L.check(L.lib.csg_conv_few_fwd(cd, _p(x), _p(w), _p(bias), _p(y), _p(ws), given, L.stream()), r["name"] + " fwd")
        torch.cuda.synchronize()
        out["y"] = y.cpu()
        if r["ws"] == "short":
            out["ws_kept"] = ws.cpu()
    if "dx" in r["dirs"]:
        dx = _owned(s["dx"], d["x_cs"], d["Cin"])
        L.check(L.lib.csg_conv_few_bwd_data(cd, _p(dy), _p(w), _p(dx), L.stream()), r["name"] + " dx")
        torch.cuda.synchronize()
        out["dx"] = dx.cpu()
    if "wgrad" in r["dirs"]:
        dw, db = _filled(s["dw"], NAN), _filled(s["db"], NAN)
        nbytes = L.lib.csg_conv_few_bwd_weight_workspace(cd)
        assert nbytes == gc.few_bwd_plan(d)["ws_bytes"], r["name"]
        ws = _filled(s["ws_wgrad"], NAN)
        L.check(L.lib.csg_conv_few_bwd_weight(cd, _p(x), _p(dy), _p(dw), _p(db), _p(ws), nbytes, L.stream()), r["name"] + " wgrad")
        torch.cuda.synchronize()
        out["dw"], out["db"] = dw.cpu(), db.cpu()
    return out


def _run(L, r, data):
    return {"nt": _run_nt, "tn": _run_tn, "few": _run_few}[r["kind"]](L, r, data)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _kept(t):
    return bool((t.view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).all())


def _judge(row, kind, name, got, ref, fp32, what=None):
    """None, or what is wrong with the owned part `got` of tensor `name`."""
    tag = "%s/%s %s" % (row["name"], kind, name)
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, expected %s" % (tag, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s: %d non-finite entries (memory no kernel wrote, or an operand no kernel may read?)" % (tag, bad)
    scale = float(ref.abs().max())
    err = float((g - ref).abs().max())
    ferr = float((fp32.double() - ref).abs().max())
    rule = "equal" if kind == "exact" else "band"
    allow = 0.0 if kind == "exact" else max(BAND * ferr, GATE * scale) + FLOOR
    _say("| %-26s | %-6s | %-3s | %-86s | scale %.2e | hip %.2e | fp32 %.2e | %s |" % (
        row["name"], kind, name, (what or gc.describe(row))[:86], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300), rule))
    if err <= allow:
        return None
    return "%s: max error %.3e, allowed %.3e (scale %.3e, fp32 error %.3e, %s; %d entries differ)" % (
        tag, err, allow, scale, ferr, rule, int(((g - ref).abs() > allow).sum()))


def _owned_part(r, name, t):
    if r["kind"] == "nt":
        return t[:, :r["N"]], t[:, r["N"]:]
    if name == "dx":
        return t[..., :r["desc"]["Cin"]], t[..., r["desc"]["Cin"]:]
    return t, None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CASES, ids=gc.case_ids())
def test_launch_rule_against_fp64(L, c, kind):
    t0 = time.time()
    r = gc.row_for(c, kind)
    data = gc.make_data(r, kind)
    runs = []
    for _ in range(2):
        _nan_fill()
        runs.append(_run(L, r, data))
    ref, fp32 = gc.reference(r, data), gc.reference(r, data, torch.float32)
    failures = []
    for name, got in runs[0].items():
        if name == "ws_kept":
            assert got is None or _kept(got), "%s: a workspace the launch may not use changed" % c["name"]
            continue
        if got is None:
            assert ref[name] is None, (c["name"], name)
            continue
        assert _same_bits(got, runs[1][name]), "%s/%s %s: a second run differs" % (c["name"], kind, name)
        own, rest = _owned_part(r, name, got)
        if rest is not None:
            assert _kept(rest), "%s/%s %s: entries outside the launch's columns changed" % (c["name"], kind, name)
        msg = _judge(r, kind, name, own, ref[name], fp32[name])
        if msg:
            failures.append(msg)
    if c["kind"] == "few":
        n = r["desc"]["cout_real"]
        for name, beyond in (("y", lambda t: t[..., n:]), ("dw", lambda t: t[n:]), ("db", lambda t: t[n:])):
            if name in runs[0] and not bool((beyond(runs[0][name]) == 0).all()):
                failures.append("%s/%s %s: entries beyond cout_real = %d are not zero: %s" % (
                    c["name"], kind, name, n, beyond(runs[0][name]).flatten()[:4].tolist()))
        if c["name"] in gc.SPLIT_TWIN and kind == "random":
            twin = gc.by_name(gc.SPLIT_TWIN[c["name"]])
            _nan_fill()
            split = _run_few(L, dict(twin, dirs=("fwd",)), data)["y"]
            assert gc.few_fwd_plan(twin["desc"])["ksplit"] > 1 and gc.few_fwd_class(c)[1] == "refused"
            scale = float(ref["y"].abs().max())
            diff = float((split.double() - runs[0]["y"].double()).abs().max())
            _say("| %-26s | %-6s | y   | unsplit against the split launch of %s: %.2e of the scale |" % (c["name"], kind, twin["name"], diff / scale))
            assert diff <= GATE * scale + FLOOR, "%s: unsplit differs from the split launch by %.3e (scale %.3e)" % (c["name"], diff, scale)
    _say("| %-26s | %-6s | time | %.2f s |" % (c["name"], kind, time.time() - t0), report=False)
    assert not failures, "\n".join(failures)


def _refused_call(L, r):
    z = lambda *shape: torch.zeros(shape, device="cuda")
    if r["entry"] == "nt":
        a, bw, y = z(r["M"], max(r["lda"], r["K"])), z(r["N"], max(r["ldb"], r["K"])), z(r["M"], max(r["ldy"], r["N"]))
        gate = z(r["M"], r["N"]) if r["gated"] else None
        return L.lib.csg_gemm_nt(gc.nt_to_ctypes(r), _p(a), _p(bw), None, _p(gate), _p(y), L.stream())
    if r["entry"] == "tn":
        M, N, K = r["M"], r["N"], r["K"]
        nbytes = L.lib.csg_gemm_tn_workspace(M, N, K)
        assert nbytes > 0
        dy, x, dw, ws = z(M, N), z(M, K), z(N, K), z(nbytes // 4)
        return L.lib.csg_gemm_tn(M, N, K, _p(dy), N, _p(x), K, _p(dw), None, _p(ws), nbytes - 4, L.stream())
    d = r["desc"]
    x, w = z(d["B"], d["IH"], d["IW"], d["x_cs"]), z(4, d["KH"], d["KW"], d["Cin"])
    y = z(d["B"], d["IH"] + 2 * d["pad"], d["IW"] + 2 * d["pad"], 4)
    if r["entry"] == "few_fwd":
        return L.lib.csg_conv_few_fwd(gc.few_to_ctypes(d), _p(x), _p(w), None, _p(y), None, 0, L.stream())
    nbytes = L.lib.csg_conv_few_bwd_weight_workspace(gc.few_to_ctypes(d))
    assert nbytes == gc.few_bwd_plan(d)["ws_bytes"] > 0
    dw, ws = z(4, d["KH"], d["KW"], d["Cin"]), z(nbytes // 4)
    return L.lib.csg_conv_few_bwd_weight(gc.few_to_ctypes(d), _p(x), _p(y), _p(dw), None, _p(ws), nbytes - 4, L.stream())


@pytest.mark.parametrize("r", REFUSALS, ids=[r["name"] for r in REFUSALS])
def test_refusals(L, r):
    with pytest.raises(RuntimeError, match=r["text"]):
        L.check(_refused_call(L, r), r["name"])
    torch.cuda.synchronize()


def _entry_run(ops, e, data):
    """{name: CPU tensor} of the entry row through ops.linear / ops.conv2d, and the launches of csrc/gemm.hip it made."""
    before = ops.gemm_calls()
    if e["kind"] == "linear":
        leaves = [data[k].clone().cuda().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2")]
        h = ops.linear(leaves[0], leaves[1], leaves[2], ops.ACT_LEAKY, 0.0, grad_is_pre=True)
        y = ops.linear(h, leaves[3], leaves[4], in_act=(ops.ACT_LEAKY, 0.0))
        names = ("dx", "dw1", "db1", "dw2", "db2")
    else:
        leaves = [data[k].clone().cuda().requires_grad_(True) for k in ("x", "w")]
        y = ops.conv2d(leaves[0], leaves[1], None, 1, 0)
        names = ("dx", "dw")
    grads = torch.autograd.grad(y, leaves, data["gy"].cuda())
    torch.cuda.synchronize()
    out = dict(zip(("y",) + names, [t.detach().cpu().contiguous() for t in (y,) + grads]))
    return out, ops.gemm_calls() - before


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("e", ENTRY_CASES, ids=[e["name"] for e in ENTRY_CASES])
def test_python_entry_against_fp64(gemm_ops, e, kind):
    """Linear -> ReLU -> Linear with the ReLU's derivative in the second layer's backward-data epilogue, and a 1x1
    convolution, at sizes the GEMM kernels only see with GEMM_MIN_TILES = 1: six and three launches of csrc/gemm.hip."""
    t0 = time.time()
    data = gc.entry_data(e, kind)
    runs = []
    for _ in range(2):
        _nan_fill()
        out, calls = _entry_run(gemm_ops, e, data)
        assert calls == e["calls"], "%s: %d launches of csrc/gemm.hip, expected %d" % (e["name"], calls, e["calls"])
        runs.append(out)
    ref, fp32 = gc.entry_ref(e, data), gc.entry_ref(e, data, torch.float32)
    failures = []
    for name, got in runs[0].items():
        assert _same_bits(got, runs[1][name]), "%s/%s %s: a second run differs" % (e["name"], kind, name)
        msg = _judge(e, kind, name, got, ref[name], fp32[name], what="ops.%s, %d launches of gemm.hip" % (e["kind"], e["calls"]))
        if msg:
            failures.append(msg)
    _say("| %-26s | %-6s | time | %.2f s |" % (e["name"], kind, time.time() - t0), report=False)
    assert not failures, "\n".join(failures)
