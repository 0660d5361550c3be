"""Authored scene graphs on a real MI355X: the box-outline kernel (csrc/overlay.hip) against its numpy restatement byte for
byte, the canonical graph without boxes against the oracle's closure of the same triplets, `Sampler.generate_from_graphs`
against `Sampler.generate` fed tensors built by hand, and the command line.

The canonical graphs expected here come from tests/canon_annotated.py, the restatement of the annotated-relationship
pipeline that calls oracle/canon.py's `path`, `hsu` and `choice_cdf`: given identical (all-zero) boxes and centres its
geometric stage derives no relation at all — every comparison of add_location_triplets is strict — so what it returns is
the closure of the authored triplets alone, which is what the device forms without reading any box."""
import json
import re

import numpy as np
import pytest
import torch

import canon_annotated as ca
import overlay_cases as oc
from conftest import load_golden
from test_authored_graphs import fixture_vocab

pytestmark = pytest.mark.gpu

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "4"]
FOUR = (0, 1, 3, 4)            # the sparse and the dense graph of three and of four objects
CASES = oc.table()


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    meta, arrays = load_golden("authored_graphs")
    return meta, arrays, fixture_vocab(meta)


# --------------------------------------------------------------------------------------------- 1. the overlay kernel
@pytest.mark.timeout(120)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_draw_boxes_u8_equals_the_restatement_byte_for_byte(cuda, ci):
    from canonicalsg2im_amd import ops
    c = CASES[ci]
    want = oc.expected(c)
    img = torch.from_numpy(c["img"]).to(cuda)
    kept = img.clone()
    args = (torch.from_numpy(c["boxes"]).to(cuda), torch.from_numpy(c["objs"]).to(cuda), c["image_id"],
            torch.from_numpy(c["palette"]).to(cuda), c["thickness"])
    got = ops.draw_boxes_u8(img, *args)
    again = ops.draw_boxes_u8(img, *args)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(img.shape) and got.data_ptr() != img.data_ptr()
    differing = int((got.cpu().numpy() != want).sum())
    print("draw_boxes_u8 %s: %d differing bytes of %d, %d painted" % (c["name"], differing, want.size,
                                                                      int((want != c["img"]).sum())))
    assert differing == 0, c["name"]
    assert torch.equal(img, kept), "the input picture was written"
    assert torch.equal(got, again), "a second call differs"


@pytest.mark.timeout(120)
def test_draw_boxes_u8_refuses_what_it_cannot_draw(cuda):
    from canonicalsg2im_amd import ops
    c = CASES[0]
    img, boxes, objs, pal = (torch.from_numpy(c[k]).to(cuda) for k in ("img", "boxes", "objs", "palette"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.draw_boxes_u8(img[..., :15], boxes, objs, 0, pal, 1)
    with pytest.raises(RuntimeError, match="thickness"):
        ops.draw_boxes_u8(img, boxes, objs, 0, pal, 0)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.draw_boxes_u8(img.float(), boxes, objs, 0, pal, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.draw_boxes_u8(img.cpu(), boxes.cpu(), objs.cpu(), 0, pal.cpu(), 1)


# --------------------------------------------------------------------------------------------- 2. canonical graph, no boxes
def _padded(arrays, vocab, which):
    """The fixture's graphs `which` as the padded batch encode_graphs makes — from the reference's arrays, by hand."""
    pad = vocab["pred_name_to_idx"]["__padding__"]
    objs = [arrays["g%d_objs" % g] for g in which]
    trip = [arrays["g%d_triplets" % g] for g in which]
    O, T = max(o.shape[0] for o in objs), max(t.shape[0] for t in trip)
    po = torch.zeros((len(which), O, objs[0].shape[1]), dtype=torch.int64)
    pt = torch.zeros((len(which), T, 3), dtype=torch.int64)
    pt[:, :, 1] = pad
    for b, (o, t) in enumerate(zip(objs, trip)):
        po[b, :o.shape[0]] = o
        pt[b, :t.shape[0]] = t
    return po, pt, torch.tensor([o.shape[0] for o in objs], dtype=torch.int64)


def _oracle_graph(objs, rows, counts, vocab, trans, conv, weights=None, uniforms=None):
    B, O = objs.shape[:2]
    return ca.canonical_batch(objs[..., 0].numpy(), np.zeros((B, O, 4), np.float32), np.zeros((B, O, 2), np.float32),
                              counts.numpy(), rows.numpy(), vocab, learned_transitivity=trans, include_dummies=False,
                              learned_converse=conv, converse_weights=weights, uniforms=uniforms)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("conv", [False, True])
@pytest.mark.parametrize("trans", [False, True])
def test_box_free_canonical_graph_equals_the_oracle_closure_of_the_same_triplets(cuda, fx, trans, conv):
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    _, arrays, vocab = fx
    objs, rows, counts = _padded(arrays, vocab, range(6))                 # every 3- and 4-object graph, hyper included
    P = len(vocab["pred_name_to_idx"])
    rng = np.random.default_rng(17)
    w = rng.normal(size=(P, P)).astype(np.float32)
    w = np.triu(w) + np.triu(w).T
    u = rng.random(200)
    want_t, want_tt, want_n, want_conv = _oracle_graph(objs, rows, counts, vocab, trans, conv, w, u)
    got_t, got_conv, got_tt = canonical_triplets(objs.to(cuda), None, None, counts, vocab, learned_transitivity=trans,
                                                 include_dummies=False, learned_converse=conv, converse_weights=w, uniforms=u,
                                                 triplets=rows)
    torch.cuda.synchronize()
    print("box-free canonical graph trans=%d conv=%d: triplets per sample %s (authored %s)" % (
        trans, conv, want_n.tolist(), [int((r[:, 1] != vocab["pred_name_to_idx"]["__padding__"]).sum()) for r in rows]))
    assert got_t.dtype == torch.int64 and tuple(got_t.shape) == want_t.shape
    assert np.array_equal(got_t.cpu().numpy(), want_t)
    assert np.array_equal(got_tt.cpu().numpy(), want_tt)
    assert np.array_equal(got_conv.cpu().numpy(), want_conv.astype(np.float32))
    if trans:
        assert int(want_tt.sum()) > 0                                     # the dense graphs' reduced edges come back as extras
    if conv:
        assert float(want_conv.sum()) > 0
    # the dummies the authored rows already carry are the ones include_dummies would add
    same = canonical_triplets(objs.to(cuda), None, None, counts, vocab, learned_transitivity=trans, include_dummies=True,
                              learned_converse=conv, converse_weights=w, uniforms=u, triplets=rows)
    assert torch.equal(same[0], got_t) and torch.equal(same[2], got_tt)
    with pytest.raises(ValueError, match="boxes=None"):
        canonical_triplets(objs.to(cuda), None, None, counts, vocab)


# --------------------------------------------------------------------------------------------- 3. the sampler, the command
@pytest.fixture(scope="module")
def drawn(cuda, fx, tmp_path_factory):
    """Fresh seeded weights at 64 x 64, saved as a checkpoint with its vocabulary; three calls of generate_from_graphs on
    the four graphs (eager, capturing, replayed).  Computed once, shared, left unchanged.  The one departure from the
    initialisation: the bias of the box head's last layer is set to a box inside the frame, so that the untrained head's
    boxes (that bias plus a small term per object) have an area and the overlay has something to draw."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    meta, arrays, vocab = fx
    opt = T.make_opt(vocab, TINY)
    torch.manual_seed(5)
    fresh = Sampler(opt, cuda)
    ckpt = {"model_state": {k: v.detach().cpu().clone() for k, v in fresh.model.state_dict().items()}, "vocab": vocab}
    last = sorted((k for k in ckpt["model_state"] if re.search(r"box_net\.\d+\.bias$", k)),
                  key=lambda k: int(re.search(r"box_net\.(\d+)\.", k).group(1)))[-1]
    assert tuple(ckpt["model_state"][last].shape) == (4,)
    ckpt["model_state"][last] = torch.tensor([0.2, 0.25, 0.45, 0.4])
    del fresh
    path = tmp_path_factory.mktemp("authored") / "fresh.pt"
    torch.save(ckpt, path)
    graphs = [meta["graphs"][g] for g in FOUR]
    s = Sampler(opt, cuda, ckpt)
    runs = [s.generate_from_graphs(graphs, overlay=True) for _ in range(3)]
    torch.cuda.synchronize()
    return {"opt": opt, "ckpt": ckpt, "path": str(path), "graphs": graphs, "runs": runs, "sampler": s}


@pytest.mark.timeout(300)
def test_generate_from_graphs_equals_generate_on_hand_built_tensors_bit_for_bit(cuda, fx, drawn):
    from canonicalsg2im_amd.sample import Sampler
    _, arrays, vocab = fx
    objs, rows, counts = _padded(arrays, vocab, FOUR)
    trip, tt, _, _ = _oracle_graph(objs, rows, counts, vocab, False, False)
    other = Sampler(drawn["opt"], cuda, drawn["ckpt"])
    want_img, want_boxes, _ = other.generate(objs.to(cuda), torch.from_numpy(trip).to(cuda), torch.from_numpy(tt).to(cuda))
    torch.cuda.synchronize()
    imgs, boxes, overlays = drawn["runs"][0]
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (4, 3, 64, 64) and tuple(boxes.shape) == (4, 5, 4)
    assert overlays.dtype == torch.uint8 and tuple(overlays.shape) == (4, 3, 64, 64)
    assert torch.equal(imgs, want_img), "%d bytes differ" % int((imgs != want_img).sum())
    assert torch.equal(boxes.view(torch.int32), want_boxes.view(torch.int32))
    for k, (i, b, o) in enumerate(drawn["runs"][1:], 1):
        assert torch.equal(i, imgs) and torch.equal(b.view(torch.int32), boxes.view(torch.int32)) and torch.equal(o, overlays), \
            "call %d differs from the eager call" % k
    s = drawn["sampler"]
    assert (s.eager_calls, s.replays) == (1, 2), (s.eager_calls, s.replays)
    assert drawn["sampler"].generate_from_graphs(drawn["graphs"])[2] is None


@pytest.mark.timeout(300)
def test_overlays_differ_from_the_pictures_only_where_the_restatement_paints(fx, drawn):
    from canonicalsg2im_amd.authored import DEFAULT_PALETTE
    _, arrays, vocab = fx
    objs, _, _ = _padded(arrays, vocab, FOUR)
    imgs, boxes, overlays = (t.cpu().numpy() for t in drawn["runs"][0])
    pal = np.asarray(DEFAULT_PALETTE, np.uint8)
    assert pal.shape == (12, 3) and len({tuple(c) for c in pal.tolist()}) == 12
    want = oc.draw_boxes(imgs, boxes, objs.numpy(), vocab["object_name_to_idx"]["__image__"], pal, 2)
    painted = np.zeros(imgs.shape, bool)
    for b in range(4):
        for o in range(boxes.shape[1]):
            if objs[b, o, 0] != 0 and oc.pixel_rect(boxes[b, o], 64, 64) is not None:
                one = oc.draw_boxes(np.zeros((1, 3, 64, 64), np.uint8), boxes[b:b + 1, o:o + 1], objs[b:b + 1, o:o + 1].numpy(), 0,
                                    np.full((1, 3), 255, np.uint8), 2)
                painted[b] |= one[0] == 255
    print("overlays: %d of %d bytes painted, %d differ from the pictures" % (int(painted.sum()), painted.size,
                                                                            int((overlays != imgs).sum())))
    assert painted.any(), "no predicted box has an area: the comparison would hold for any overlay"
    assert not (overlays != imgs)[~painted].any()
    assert np.array_equal(overlays, want)


@pytest.mark.timeout(300)
def test_command_line_writes_pictures_layouts_and_graphs(cuda, fx, drawn, tmp_path, capsys):
    from PIL import Image

    from canonicalsg2im_amd.scripts import sample as cli
    _, _, vocab = fx
    src = tmp_path / "graphs.json"
    src.write_text(json.dumps(drawn["graphs"]))
    out = tmp_path / "out"
    cli.main(["--scene_graphs", str(src), "--output_dir", str(out), "--checkpoint_name", drawn["path"], "--num_samples", "99"]
             + TINY)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(r"4 images in [\d.]+ s  \[[\d.]+ img/s\]  \(\d+ replayed, \d+ eager calls\)", line), line
    imgs, _, overlays = drawn["runs"][0]
    assert sorted(p.name for p in out.iterdir()) == sorted(
        ["graphs.json"] + ["img_%06d_%s.png" % (i, k) for i in range(4) for k in ("generated", "layout")])
    for i in range(4):
        for kind, t in (("generated", imgs), ("layout", overlays)):
            png = np.asarray(Image.open(out / ("img_%06d_%s.png" % (i, kind))))
            assert png.dtype == np.uint8 and np.array_equal(png, t[i].permute(1, 2, 0).cpu().numpy()), (i, kind)
    written = json.loads((out / "graphs.json").read_text())
    assert len(written) == 4 and written[0]["objects"] == drawn["graphs"][0]["objects"]
    names = {t[1] for g in written for t in g["triplets"]}
    assert names == {"front", "right", "__in_image__"}, names
    assert written[0]["triplets"][-3:] == [[i, "__in_image__", 3] for i in range(3)]
    # --draw_boxes 0: no layout pictures
    bare = tmp_path / "bare"
    cli.main(["--scene_graphs", str(src), "--output_dir", str(bare), "--checkpoint_name", drawn["path"], "--draw_boxes", "0"]
             + TINY)
    assert sorted(p.name for p in bare.iterdir()) == sorted(["graphs.json"] + ["img_%06d_generated.png" % i for i in range(4)])
    # a checkpoint without a vocabulary, and none at all
    novocab = tmp_path / "novocab.pt"
    torch.save({"model_state": drawn["ckpt"]["model_state"]}, novocab)
    with pytest.raises(SystemExit, match="no vocabulary"):
        cli.main(["--scene_graphs", str(src), "--checkpoint_name", str(novocab)] + TINY)
    with pytest.raises(SystemExit, match="--checkpoint_name"):
        cli.main(["--scene_graphs", str(src)] + TINY)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps([drawn["graphs"][0], {"objects": [], "relationships": {}}]))
    with pytest.raises(SystemExit, match="scene graph 1"):
        cli.main(["--scene_graphs", str(bad), "--checkpoint_name", drawn["path"]] + TINY)


@pytest.mark.timeout(300)
def test_command_line_without_the_flag_prints_the_old_line(cuda, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import sample as cli
    cli.main(TINY[:-2] + ["--batch_size", "2", "--num_samples", "2", "--output_dir", str(tmp_path / "plain")])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(r"2 images in [\d.]+ s  \[[\d.]+ img/s\]  \(\d+ replayed, \d+ eager calls\)", line), line
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["img_000000.png", "img_000001.png"]
