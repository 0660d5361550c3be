"""The first launch of a kernel in a process is the one that raises its dynamic LDS limit (csg::lds_limit, csg_common.h):
once per kernel and device, to the largest size the kernel's launch rule can ask for.  What a once-flag can get wrong is
the first request being the biggest one, so a fresh child process makes the FIRST call of each converted entry its
largest-LDS shape from the path tables (no small warm-up before it), and every call must return CSG_OK and agree bit for
bit with a second call.  Every shape is one the suite runs elsewhere against fp64; nothing is compared to a reference
here.  On a runtime that lets an unraised request through, no entry can tell a missing raise from a present one: what
is held is that the raise succeeds on the first call and that the largest request then runs and repeats."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout_fwd(L, ops):
    """lay_s1024_32 (tests/geom_cases.py): k_layout_fwd_rows with 137 232 bytes."""
    B, O, S, H = 2, 6, 1024, 32
    g = torch.Generator().manual_seed(1)
    vecs = torch.randn(B, O, S, generator=g).cuda()
    lo = torch.rand(B, O, 2, generator=g) * 0.5
    boxes = torch.cat([lo, lo + 0.1 + torch.rand(B, O, 2, generator=g) * 0.4], -1).cuda()
    valid = torch.ones(B, O, dtype=torch.uint8).cuda()
    out = torch.full((B, H, H, S), float("nan"), device="cuda")
    L.check(L.lib.csg_layout_fwd(L.ptr(vecs), L.ptr(boxes), L.ptr(valid), None, 0, B, O, S, H, H, H, H, L.ptr(out), S, 0,
                                 L.stream()), "layout_fwd")
    return [out]


def _layout_bwd_masks(L, ops):
    """lay_m1_soft_mixed: the masked backward with the longest coverage rows of the table (64 x 64).  That is 1 568 bytes:
    this entry exercises the call that raises the limit to its 102 400-byte cap, not a request that needs it."""
    B, O, S, H, M = 2, 12, 8, 64, 1
    g = torch.Generator().manual_seed(2)
    vecs = torch.randn(B, O, S, generator=g).cuda()
    lo = torch.rand(B, O, 2, generator=g) * 0.5
    boxes = torch.cat([lo, lo + 0.1 + torch.rand(B, O, 2, generator=g) * 0.4], -1).cuda()
    valid = torch.ones(B, O, dtype=torch.uint8).cuda()
    dout = torch.randn(B, H, H, S, generator=g).cuda()
    dmasks = torch.full((B, O, M, M), float("nan"), device="cuda")
    L.check(L.lib.csg_layout_bwd_masks(L.ptr(dout), S, 0, L.ptr(boxes), L.ptr(valid), M, B, O, S, H, H, H, H, L.ptr(vecs),
                                       L.ptr(dmasks), 0, L.stream()), "layout_bwd_masks")
    return [dmasks]


def _csr_sorted(L, ops):
    """csr_o3_t65535 (tests/graph_cases.py): the counting sort at its largest admitted T, 131 878 bytes."""
    B, T, O = 2, 65535, 3
    assert L.lib.csg_graph_csr_lds(T, O) == 2 * O * 64 * 2 + (3 * O + 1) * 4 + 2 * T
    g = torch.Generator().manual_seed(3)
    tr = torch.stack([torch.randint(0, O, (B, T), generator=g), torch.randint(0, 5, (B, T), generator=g),
                      torch.randint(0, O, (B, T), generator=g)], -1).cuda()
    row_ptr = torch.full((B, O + 1), -1, dtype=torch.int32, device="cuda")
    col = torch.full((B, 2 * T), -1, dtype=torch.int32, device="cuda")
    L.check(L.lib.csg_graph_csr_build(L.ptr(tr), B, T, O, L.ptr(row_ptr), L.ptr(col), L.stream()), "graph_csr_build")
    return [row_ptr, col]


def _conv_fwd_bn128(L, ops):
    """bn128 (tests/igemm_cases.py): csg_conv_fwd with the 128-wide block, 73 920 bytes."""
    g = torch.Generator().manual_seed(4)
    x = ops.nhwc(torch.randn(2, 8, 5, 7, generator=g).cuda())
    wp = torch.randn(128, 3, 3, 8, generator=g).cuda()
    with torch.no_grad():
        return [ops.conv2d_forward(x, wp, torch.randn(128, generator=g).cuda(), 3, 3, 1, (1, 1))]


def _wino_desc(L, B, H, W, Cin, Cout):
    d = L.WinoDesc()
    d.B, d.H, d.W, d.Cin, d.x_cs, d.Cout, d.y_cs, d.act, d.slope = B, H, W, Cin, Cin, Cout, Cout, 0, 0.0
    return d


def _wino4_persistent(L, ops):
    """PERSISTENT_SHAPES[0] (tests/test_gpu_wino4.py): k_wino4_conv_v<4, true>, one block per CU."""
    B, Cin, Cout, H, W = 2, 32, 512, 128, 128
    g = torch.Generator().manual_seed(5)
    x = ops.nhwc(torch.randn(B, Cin, H, W, generator=g).cuda())
    up = ops.wino_pack((torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)).cuda(), False, None, 4)
    bias = torch.randn(Cout, generator=g).cuda()
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    d = _wino_desc(L, B, H, W, Cin, Cout)
    assert L.lib.csg_wino4_supported(d) == 1 and L.lib.csg_wino4_persistent(-1) != 0
    L.check(L.lib.csg_wino4_conv(d, L.ptr(x), L.ptr(up), L.ptr(bias), None, None, 0.0, L.ptr(y), None, 0, L.stream()),
            "wino4_conv")
    return [y]


def _wino4_wgrad(L, ops):
    """WG_SHAPES[0] (tests/test_gpu_wino4.py): csg_wino4_bwd_weight; its LDS size is the same for every shape."""
    B, Cin, Cout, H, W = 2, 64, 64, 8, 8
    g = torch.Generator().manual_seed(6)
    x, dy = ops.nhwc(torch.randn(B, Cin, H, W, generator=g).cuda()), ops.nhwc(torch.randn(B, Cout, H, W, generator=g).cuda())
    d = _wino_desc(L, B, H, W, Cin, Cout)
    nbytes = L.lib.csg_wino4_bwd_weight_workspace(d)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, device="cuda")
    dw = torch.full((Cout, 3, 3, Cin), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    L.check(L.lib.csg_wino4_bwd_weight(d, L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(db), L.ptr(ws), nbytes, L.stream()), "wino4_bwd_weight")
    return [dw, db]


ENTRIES = [_layout_fwd, _layout_bwd_masks, _csr_sorted, _conv_fwd_bn128, _wino4_persistent, _wino4_wgrad]


def _child():
    from canonicalsg2im_amd import _lib as L, ops
    for fn in ENTRIES:
        first = [t.clone() for t in fn(L, ops)]          # check() raises unless the entry returned CSG_OK
        second = fn(L, ops)
        torch.cuda.synchronize()
        assert len(first) == len(second) and first
        for a, b in zip(first, second):
            assert bool(torch.isfinite(a.float()).all()), fn.__name__      # every entry the kernels own was written
            assert a.dtype == b.dtype and torch.equal(a, b), fn.__name__
        print("ok", fn.__name__, flush=True)


@pytest.mark.gpu
def test_first_launch_with_the_largest_lds_in_a_fresh_process():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert [l.split()[1] for l in r.stdout.splitlines() if l.startswith("ok ")] == [fn.__name__ for fn in ENTRIES]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child()
