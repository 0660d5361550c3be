"""Scene-graph pictures on a real MI355X: the rasteriser (csg_draw_graph_u8, csrc/overlay.hip) against its numpy
restatement (tests/sgdraw_cases.py) byte for byte, `sgdraw.draw_scene_graphs` against the restatement of its own layout, and
`scripts.sample --draw_scene_graphs 0|1|2` in fresh processes against what the library calls give.

No tolerance anywhere: every comparison is of bytes.  Shapes: the table's canvases of 16 x 16 up to 40 x 136 (three tiles
by three) and one picture of 4096 records; seeded random weights at 64 x 64 as tests/test_gpu_labels.py builds them, four
authored graphs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgdraw_cases as sc
from conftest import load_golden
from test_authored_graphs import fixture_vocab
from test_gpu_labels import FOUR, TINY, _checkpoint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.table()
MODEL = TINY + ["--learned_transitivity", "1"]           # the canonical graph gets transitive edges: mode 2 has colours to show


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _font():
    from canonicalsg2im_amd.font5x7 import FONT
    return FONT


# --------------------------------------------------------------------------------------------- 1. the rasteriser
@pytest.mark.timeout(120)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_draw_graph_u8_equals_the_restatement_byte_for_byte(cuda, ci):
    from canonicalsg2im_amd import ops
    c = CASES[ci]
    want = sc.expected(c, _font())
    args = (c["prims"], c["prim_off"], c["text"], c["H"], c["W"], c["background"])
    got = ops.draw_graph_u8(*args, device=cuda)
    into = torch.full_like(got, 77)
    again = ops.draw_graph_u8(*args, font=torch.from_numpy(_font().copy()).to(cuda), out=into)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.device == cuda
    differing = int((got.cpu().numpy() != want).sum())
    print("draw_graph_u8 %s: %d differing bytes of %d, %d painted" % (
        c["name"], differing, want.size, int((want != np.asarray(c["background"], np.uint8)[None, :, None, None]).any(1).sum())))
    assert differing == 0, c["name"]
    assert again.data_ptr() == into.data_ptr() and torch.equal(got, again), "a second call, into a given buffer, differs"


@pytest.mark.timeout(120)
def test_draw_graph_u8_refuses_what_the_entry_point_cannot_paint(cuda):
    from canonicalsg2im_amd import _lib, ops
    c = CASES[0]
    args = (c["prims"], c["prim_off"], c["text"])
    with pytest.raises(RuntimeError, match="W a multiple of 4"):
        ops.draw_graph_u8(*args, 16, 18, sc.WHITE, device=cuda)
    with pytest.raises(RuntimeError, match=r"\[1, 2048\]"):
        ops.draw_graph_u8(*args, 2049, 16, sc.WHITE, device=cuda)
    with pytest.raises(RuntimeError, match=r"\[1, 2048\]"):
        ops.draw_graph_u8(*args, 16, 0, sc.WHITE, device=cuda)
    with pytest.raises(RuntimeError, match=r"font must be uint8 \(95, 7\)"):
        ops.draw_graph_u8(*args, 16, 16, sc.WHITE, font=torch.zeros((95, 8), dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError, match="out must be a contiguous uint8"):
        ops.draw_graph_u8(*args, 16, 16, sc.WHITE, out=torch.zeros((1, 3, 16, 20), dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.draw_graph_u8(*args, 16, 16, sc.WHITE, device="cpu")
    with pytest.raises(ValueError, match="a coordinate outside"):
        ops.draw_graph_u8([sc.seg(0, 0, 5000, 0, sc.RED)], [0, 1], b"", 16, 16, sc.WHITE, device=cuda)
    # the C entry itself, before any launch: B < 1, H and W outside [1, 2048], W % 4, a null pointer
    p = torch.zeros(64, dtype=torch.uint8, device=cuda)
    a = _lib.ptr(p)
    call = _lib.lib.csg_draw_graph_u8
    assert _lib.lib.csg_version() == 122
    for B, H, W in ((0, 16, 16), (1, 0, 16), (1, 2049, 16), (1, 16, 2052), (1, 16, 18)):
        assert call(a, 0, a, a, 0, a, B, H, W, 0, a, None) == -1 and "csg_draw_graph_u8: bad shape" in _lib.last_error()
    for k in range(5):
        ptrs = [None if i == k else a for i in range(5)]
        assert call(ptrs[0], 0, ptrs[1], ptrs[2], 0, ptrs[3], 1, 4, 4, 0, ptrs[4], None) == -1
        assert "null operand" in _lib.last_error()
    names = [_lib.lib.csg_prof_kernel_name(k).decode() for k in range(_lib.lib.csg_prof_num_kernels())]
    assert "draw_graph_u8" in names


# --------------------------------------------------------------------------------------------- 2. laid-out graphs
@pytest.fixture(scope="module")
def fx():
    meta, _ = load_golden("authored_graphs")
    return meta, fixture_vocab(meta)


@pytest.mark.timeout(120)
def test_draw_scene_graphs_paints_every_graph_at_its_own_size_in_one_launch(cuda, fx):
    from canonicalsg2im_amd import _lib, authored, sgdraw
    meta, vocab = fx
    graphs = authored.load_graphs(meta["graphs"], vocab)
    sizes, prims, off, text = sgdraw.layout_batch(graphs, vocab)
    H, W = max(h for _, h in sizes), max(w for w, _ in sizes)
    want = sc.draw_graph(prims, off, text, H, W, sgdraw.DEFAULT_STYLE["background"], _font())
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        pics = sgdraw.draw_scene_graphs(graphs, vocab, cuda)
        launches = _lib.prof_read()
    finally:
        _lib.prof_enable(0)
    assert launches["draw_graph_u8"][1] == 1 and set(launches) == {"draw_graph_u8"}, launches
    assert len(pics) == 12 and len({p.untyped_storage().data_ptr() for p in pics}) == 1          # views of one canvas
    for g, (p, (w, h)) in enumerate(zip(pics, sizes)):
        assert p.dtype == torch.uint8 and tuple(p.shape) == (3, h, w) and w % 4 == 0
        assert np.array_equal(p.cpu().numpy(), want[g, :, :h, :w]), g
        assert (want[g, :, h:, :] == 255).all() and (want[g, :, :, w:] == 255).all()           # nothing beyond its own size
    assert len(set(sizes)) > 1
    print("scene graphs: sizes %s, %d records, %d text bytes, canvas %d x %d" % (sizes, len(prims), len(text), H, W))
    # edge types: host lists and device tensors give the same bytes, which differ from the one-colour picture
    rows = authored.encode_graphs(graphs, vocab)[1]
    types = (torch.arange(rows.shape[1]) % 3).expand(rows.shape[0], -1).contiguous()
    typed = sgdraw.draw_scene_graphs(graphs, vocab, cuda, rows, types)
    device = sgdraw.draw_scene_graphs(graphs, vocab, cuda, rows.to(cuda), types.to(cuda))
    assert all(torch.equal(a, b) for a, b in zip(typed, device))
    assert all(a.shape == b.shape for a, b in zip(typed, pics)) and not torch.equal(typed[4], pics[4])
    with pytest.raises(ValueError, match="scene graph 1: the picture's height would be"):
        sgdraw.draw_scene_graphs(graphs[:2], vocab, cuda, [rows[0].tolist(), [[0, 1, 1]] * 90])


# --------------------------------------------------------------------------------------------- 3. the command line
def _run(code_or_module, argv, timeout=180):
    cmd = [sys.executable] + code_or_module + argv
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def runs(cuda, fx, tmp_path_factory):
    """One checkpoint, three fresh processes (--draw_scene_graphs 0, 1 and 2) and the library's own calls on the same
    graphs.  The run with 0 goes through `python -c` so that it can say whether sgdraw was ever imported.  Computed once,
    shared, left unchanged."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    meta, vocab = fx
    opt = T.make_opt(vocab, MODEL)
    ckpt = _checkpoint(opt, cuda, vocab)
    tmp = tmp_path_factory.mktemp("sgdraw")
    path = tmp / "fresh.pt"
    torch.save(ckpt, path)
    graphs = [meta["graphs"][g] for g in FOUR]
    src = tmp / "graphs.json"
    src.write_text(json.dumps(graphs))
    argv = ["--scene_graphs", str(src), "--checkpoint_name", str(path)] + MODEL
    never = ("import sys; from canonicalsg2im_amd.scripts import sample; sample.main(sys.argv[1:]); "
             "assert 'canonicalsg2im_amd.sgdraw' not in sys.modules, 'sgdraw was imported'")
    _run(["-c", never], argv + ["--output_dir", str(tmp / "out0")])
    _run(["-m", "canonicalsg2im_amd.scripts.sample"], argv + ["--output_dir", str(tmp / "out1"), "--draw_scene_graphs", "1"])
    _run(["-m", "canonicalsg2im_amd.scripts.sample"], argv + ["--output_dir", str(tmp / "out2"), "--draw_scene_graphs", "2"])
    s = Sampler(opt, cuda, ckpt)
    plain = s.generate_from_graphs(graphs, overlay=True)
    off = s.generate_from_graphs(graphs, overlay=True, return_graph=False)
    on = s.generate_from_graphs(graphs, overlay=True, return_graph=True)
    torch.cuda.synchronize()
    return {"tmp": tmp, "graphs": graphs, "vocab": vocab, "plain": plain, "off": off, "on": on}


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


@pytest.mark.timeout(600)
def test_flag_0_and_return_graph_false_change_no_file_and_no_tensor(cuda, runs):
    tmp = runs["tmp"]
    base = sorted(os.listdir(tmp / "out0"))
    assert base == sorted(["graphs.json"] + ["img_%06d_%s.png" % (i, k) for i in range(4) for k in ("generated", "layout")])
    for mode in (1, 2):                                  # the other runs write the same bytes under those names
        for name in base:
            assert (tmp / ("out%d" % mode) / name).read_bytes() == (tmp / "out0" / name).read_bytes(), (mode, name)
    assert len(runs["plain"]) == len(runs["off"]) == 3 and len(runs["on"]) == 4
    for k in range(3):
        assert torch.equal(runs["plain"][k], runs["off"][k]) and torch.equal(runs["plain"][k], runs["on"][k]), k
    imgs, _, overlays = runs["plain"]
    for i in range(4):
        for kind, t in (("generated", imgs), ("layout", overlays)):
            assert np.array_equal(_png(tmp / "out0" / ("img_%06d_%s.png" % (i, kind))), t[i].permute(1, 2, 0).cpu().numpy())


@pytest.mark.timeout(600)
def test_command_line_writes_each_graph_picture_at_its_own_size(cuda, runs):
    from canonicalsg2im_amd import sgdraw
    tmp, graphs, vocab = runs["tmp"], runs["graphs"], runs["vocab"]
    extra = ["img_%06d_sg.png" % i for i in range(4)]
    for mode in (1, 2):
        assert sorted(set(os.listdir(tmp / ("out%d" % mode))) - set(os.listdir(tmp / "out0"))) == extra
    triplets, triplet_type = runs["on"][3]
    assert triplets.is_cuda and triplets.dtype == torch.int64 and triplets.dim() == 3 and triplets.shape[2] == 3
    assert tuple(triplet_type.shape) == tuple(triplets.shape[:2]) and int((triplet_type == sgdraw.TRANSITIVE).sum()) > 0
    host = sgdraw.draw_scene_graphs(graphs, vocab, cuda)
    canon = sgdraw.draw_scene_graphs(graphs, vocab, cuda, triplets, triplet_type)
    shapes = set()
    for i in range(4):
        for mode, pics in ((1, host), (2, canon)):
            png = _png(tmp / ("out%d" % mode) / extra[i])
            assert png.shape == (pics[i].shape[1], pics[i].shape[2], 3), (mode, i, png.shape)
            assert np.array_equal(png, pics[i].permute(1, 2, 0).cpu().numpy()), (mode, i)
            shapes.add(png.shape)
    assert len(shapes) > 1
    # the canonical picture shows edges the host-encoded one does not have, in the transitive colour
    green = np.asarray(sgdraw.DEFAULT_STYLE["types"][sgdraw.TRANSITIVE][0], np.uint8)
    seen = [bool((p.permute(1, 2, 0).cpu().numpy() == green).all(-1).any()) for p in canon]
    assert any(seen) and not any(bool((p.permute(1, 2, 0).cpu().numpy() == green).all(-1).any()) for p in host)
