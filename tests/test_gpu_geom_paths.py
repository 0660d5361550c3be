"""Every layout, mask, paint and crop kernel path through the entry point the model uses (`ops.layout_pyramid`,
`ops.disc_input`, `ops.layout_paint`, `ops.crop_objects`, and the C ABI's channel slice) on a real MI355X, against the
float64 restatement of the contract (tests/geom_cases.py: the table and `geom_ref64`).

Per row: the allocator's free blocks are filled with NaN before each run, so an output pixel, a partial slot or a gradient
a kernel never writes shows up as NaN; every output and every requested gradient must be finite and of the expected shape,
a gradient not asked for must be None, a masked-out object's gradients exactly 0, disc_input's image channels bit-exact and
its pad channels exactly 0, and a second run must reproduce every tensor bit for bit (README: every reduction is an ordered
sum).

Gates.  Outputs, the vecs gradient and the image gradient: max error <= 1e-5 of the fp64 tensor's largest entry plus a 1e-6
floor (the gate of the conv plans).  Box and mask gradients sum O(H W) border terms scaled by n / size, so no fixed
fraction can be derived for them: they are held against the float32 CPU evaluation of the same oracle function on the same
inputs, hip_err <= max(3 x fp32_oracle_err, 1e-5 x scale) + 1e-6 (3: fp64_band.Band's factor for "within the reference
arithmetic's own noise").  The measured pairs of every row are in profiles/geom_paths_gpu.txt.  Paint rows use the output
gate: their rows keep clear of the mass order's and the threshold's discontinuities (tests/test_geom_cases.py)."""
import os
import sys
import time

import pytest
import torch

import geom_cases as gc
from geom_cases import CASES, case_ids
from test_gpu_conv_plans import _nan_fill

pytestmark = pytest.mark.gpu
GATE, FLOOR, BAND = 1e-5, 1e-6, 3.0
BANDED = ("dboxes", "dmasks")
REPORT = os.environ.get("GEOM_PATHS_REPORT")          # a file that receives the table too (profiles/geom_paths_gpu.txt)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops as o
    return o


HEADER = """tests/test_gpu_geom_paths.py on an MI355X (gfx950): one line per row and tensor - the kernels the launch rules give the
row, the largest fp64 entry (scale), the HIP error and the float32 CPU oracle's error on the same inputs, both as fractions
of the scale, and the rule the tensor is held to: gate = 1e-5 of the scale + 1e-6; band = max(3 x fp32 oracle error, 1e-5
of the scale) + 1e-6 (box and mask gradients).  Written by the test itself when GEOM_PATHS_REPORT names a file.
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


def _dev(t, grad=False):
    return t.to(torch.float32).cuda().requires_grad_(grad)


def _masks(c, d, grad):
    if d["masks"] is None:
        return None
    return d["masks"].cuda() if not d["masks"].is_floating_point() else _dev(d["masks"], grad)


def _run(ops, c, d):
    """One forward (+ backward) of row `c`: {tensor name: device tensor or None}, named like geom_cases.evaluate."""
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    need = c["need"]
    if c["family"] == "crop":
        img, boxes = _dev(d["img"], "img" in need), _dev(d["boxes"], "boxes" in need)
        out = ops.crop_objects(img, boxes, d["img_idx"].cuda(), c["HH"])
        if need:
            out.backward(_dev(d["dout"]))
        return dict(out0=out, dimg=img.grad, dboxes=boxes.grad)
    B, O, S, H, W = c["B"], c["O"], c["S"], c["H"], c["W"]
    vecs, boxes = _dev(d["vecs"], "vecs" in need), _dev(d["boxes"], "boxes" in need)
    valid = d["valid"].to(torch.uint8).cuda()
    masks = _masks(c, d, "masks" in need)
    if c["entry"] == "layout_paint":
        outs = ops.layout_paint(vecs, boxes, valid, masks, H, c["sizes"], W=W)
        return dict({"out%d" % i: o for i, o in enumerate(outs)}, dvecs=None, dboxes=None, dmasks=None)
    if c["entry"] == "layout_pyramid":
        outs = ops.layout_pyramid(vecs, boxes, valid, H, c["sizes"], masks=masks, W=W)
        torch.autograd.backward(outs, [_dev(g) for g in d["douts"]])
        return dict({"out%d" % i: o for i, o in enumerate(outs)}, dvecs=vecs.grad, dboxes=boxes.grad,
                    dmasks=None if masks is None else masks.grad)
    if c["entry"] == "disc_input":
        img = _dev(d["img"])
        if c["img_fmt"] == "cl":
            img = img.contiguous(memory_format=torch.channels_last)
        img.requires_grad_("img" in need)
        buf = ops.disc_input(img, vecs, boxes, valid, H, masks=masks)
        buf.backward(_dev(d["douts"][0]))
        return dict(out0=buf, dvecs=vecs.grad, dboxes=boxes.grad, dmasks=None if masks is None else masks.grad, dimg=img.grad)
    # abi_slice: the layout is channels [off, off + S) of a pixel of `cs` floats; so is the incoming gradient
    (h, w), cs, off = c["sizes"][0], c["out_cs"], c["out_off"]
    vecs, boxes = vecs.detach(), boxes.detach()
    mk = None if masks is None else masks.detach().to(torch.float32).contiguous()
    M = 0 if mk is None else int(mk.shape[-1])
    buf = torch.full((B, h, w, cs), gc.SENTINEL, device="cuda")
    check(lib.csg_layout_fwd(ptr(vecs), ptr(boxes), ptr(valid), ptr(mk), M, B, O, S, H, W, h, w, ptr(buf), cs, off, stream()),
          "layout_fwd")
    rest = torch.cat([buf[..., :off], buf[..., off + S:]], -1)
    assert bool((rest == gc.SENTINEL).all()), "%s: the forward wrote outside its channel slice" % c["name"]
    gbuf = torch.full((B, h, w, cs), float("nan"), device="cuda")
    gbuf[..., off:off + S] = _dev(d["douts"][0]).permute(0, 2, 3, 1)
    dvecs = torch.full((B, O, S), float("nan"), device="cuda")
    dboxes = torch.full((B, O, 4), float("nan"), device="cuda") if "boxes" in need else None
    nws = lib.csg_layout_bwd_workspace(B, O, S, h, w, 0 if mk is None else 1, 0 if dboxes is None else 1)
    assert (nws > 0) == (gc.level_rules(c)[0]["bwd"] == "tiled"), c["name"]
    ws = torch.empty(nws // 4, device="cuda") if nws > 0 else None
    check(lib.csg_layout_bwd(ptr(gbuf), cs, off, ptr(boxes), ptr(valid), ptr(mk), M, B, O, S, H, W, h, w, ptr(dvecs), 0,
                             ptr(vecs), ptr(dboxes), ptr(ws), nws, stream()), "layout_bwd")
    return dict(out0=buf[..., off:off + S].permute(0, 3, 1, 2), dvecs=dvecs, dboxes=dboxes, dmasks=None)


def _judge(c, name, got, ref, fp32):
    g = got.double()
    assert tuple(g.shape) == tuple(ref.shape), "%s %s: shape %s, expected %s" % (c["name"], name, tuple(g.shape), tuple(ref.shape))
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, "%s %s: %d non-finite entries (memory no kernel wrote?)" % (c["name"], name, bad)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((g - ref).abs().max()) if ref.numel() else 0.0
    ferr = float((fp32.double() - ref).abs().max()) if ref.numel() else 0.0
    banded = name in BANDED
    allow = (max(BAND * ferr, GATE * scale) if banded else GATE * scale) + FLOOR
    _say("| %-24s | %-6s | %-46s | scale %.2e | hip %.2e | fp32 oracle %.2e | %s |" % (
        c["name"], name, " ".join(c["kernels"])[:46], scale, err / max(scale, 1e-300), ferr / max(scale, 1e-300),
        "band" if banded else "gate"))
    return None if err <= allow else "%s %s: max error %.3e, allowed %.3e (scale %.3e, fp32 oracle error %.3e)" % (
        c["name"], name, err, allow, scale, ferr)


@pytest.mark.parametrize("c", CASES, ids=case_ids())
def test_path_against_fp64(ops, c):
    t0 = time.time()
    d = gc.make_data(c)
    if c["refuse"]:
        img, boxes = _dev(d["img"], "img" in c["need"]), _dev(d["boxes"], "boxes" in c["need"])
        with pytest.raises(RuntimeError, match=c["refuse"]):
            ops.crop_objects(img, boxes, d["img_idx"].cuda(), c["HH"])
        return
    runs = []
    for _ in range(2):
        _nan_fill()
        o = _run(ops, c, d)
        torch.cuda.synchronize()
        runs.append({t: (None if v is None else v.detach().cpu().clone()) for t, v in o.items()})
    ref = gc.geom_ref64(c, d)
    fp32 = gc.evaluate(c, d, gc.ORACLE, torch.float32)
    assert set(ref) == set(runs[0]), sorted(set(ref) ^ set(runs[0]))
    failures = []
    for name, r in ref.items():
        got = runs[0][name]
        if r is None:
            assert got is None, "%s: %s was not asked for and came back" % (c["name"], name)
            continue
        assert got is not None, "%s: %s was asked for and did not come back" % (c["name"], name)
        msg = _judge(c, name, got, r, fp32[name])
        if msg:
            failures.append(msg)
        assert torch.equal(got, runs[1][name]), "%s %s: a second run differs (max %.3e)" % (
            c["name"], name, float((got - runs[1][name]).abs().max()))
    if c["family"] == "layout":
        off = ~d["valid"]
        for name in ("dvecs", "dboxes", "dmasks"):
            got = runs[0].get(name)
            if got is not None and bool(off.any()):
                assert float(got[off].abs().max()) == 0.0, "%s: %s of a masked-out object is not exactly 0" % (c["name"], name)
    if c["entry"] == "disc_input":
        S, buf = c["S"], runs[0]["out0"]
        assert torch.equal(buf[:, S:S + 3], d["img"].to(torch.float32)), "%s: the image channels are not bit-exact" % c["name"]
        assert float(buf[:, S + 3:].abs().max()) == 0.0, "%s: the pad channels are not 0" % c["name"]
    _say("| %-24s | time   | %.2f s |" % (c["name"], time.time() - t0), report=False)
    assert not failures, "\n".join(failures)
