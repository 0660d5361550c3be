"""The CPU oracle against the golden vectors produced by the real reference
(tests/golden/make_golden.py).  fp32 tolerance: rtol 1e-4 (BASELINE.json north_star)."""
import torch

import oracle
from oracle.fp64 import generated_image64
from canonicalsg2im_amd.scripts.args import make_opt
from canonicalsg2im_amd.synth import make_vocab
from conftest import assert_close, load_golden, state_from_shapes, sub_state

RTOL, ATOL = 1e-4, 2e-6


def test_layout_forward_backward():
    meta, a = load_golden("layout")
    for H, W in meta["sizes"]:
        tag = "%dx%d" % (H, W)
        vecs = a["vecs"].clone().requires_grad_(True)
        boxes = a["boxes"].clone().requires_grad_(True)
        out = oracle.boxes_to_layout(vecs, boxes, H, W)
        assert_close(out, a["out_" + tag], RTOL, ATOL, "layout " + tag)
        gv, gb = torch.autograd.grad((out * a["w_" + tag]).sum(), [vecs, boxes])
        assert_close(gv, a["gvecs_" + tag], RTOL, 1e-5, "layout dvecs " + tag)
        assert_close(gb, a["gboxes_" + tag], 1e-3, 1e-3, "layout dboxes " + tag)


def test_graph_triple_conv():
    meta, a = load_golden("gconv")
    st = sub_state(a, "sd:")
    w_trans = st.pop("predicates_transitive_weights")
    obj = a["obj"].clone().requires_grad_(True)
    pred = a["pred"].clone().requires_grad_(True)
    new_obj, new_p = oracle.graph_triple_conv(st, "", obj, pred, a["edges"], a["p"] != 0, a["tt"], a["p"], w_trans)
    assert_close(new_obj, a["new_obj"], RTOL, ATOL, "new_obj")
    assert_close(new_p, a["new_p"], RTOL, ATOL, "new_p")
    ((new_obj * a["wo"]).sum() + (new_p * a["wp"]).sum()).backward()
    assert_close(obj.grad, a["gobj"], RTOL, 1e-5, "dobj")
    assert_close(pred.grad, a["gpred"], RTOL, 1e-5, "dpred")
    assert_close(w_trans.grad, a["grad:predicates_transitive_weights"], RTOL, 1e-5, "dw_trans")
    for k, v in st.items():
        assert_close(v.grad, a["grad:" + k], RTOL, 1e-5, "d" + k)


def _check_sg2layout(tag):
    meta, a = load_golden("sg2layout_" + tag)
    vocab = make_vocab(meta["vocab"])
    st = sub_state(a, "sd:")
    # the reference registers ONE Parameter under six names (model.py:32,45; graph.py:42)
    w = st["trans_candidates_weights"]
    for k in list(st):
        if k.endswith("predicates_transitive_weights"):
            st[k] = w
    obj_vecs, boxes_pred, _ = oracle.sg2layout_forward(st, vocab, a["objs"], a["triplets"], a["tt"])
    assert_close(obj_vecs, a["obj_vecs"], RTOL, ATOL, "obj_vecs")
    assert_close(boxes_pred, a["boxes_pred"], RTOL, ATOL, "boxes_pred")
    ((obj_vecs * a["wv"]).sum() + (boxes_pred * a["wb"]).sum()).backward()
    n = 0
    for k, v in st.items():
        if ("grad:" + k) in a and v.grad is not None:
            assert_close(v.grad, a["grad:" + k], RTOL, 1e-5, "d" + k)
            n += 1
    assert n > 10


def test_sg2layout_single_attribute():
    _check_sg2layout("a1")


def test_sg2layout_clevr_attributes():
    _check_sg2layout("a4")


def test_spade_resblock_train_and_eval():
    meta, a = load_golden("spade_block")
    st = state_from_shapes(meta["shapes"], seed=3)
    x = a["x"].clone().requires_grad_(True)
    seg = a["seg"].clone().requires_grad_(True)
    y = oracle.spade_resblock(st, "", x, seg, training=True)
    assert_close(y, a["y"], RTOL, 1e-5, "block out")
    (y * a["w"]).sum().backward()
    assert_close(x.grad, a["gx"], RTOL, 1e-5, "dx")
    assert_close(seg.grad, a["gseg"], RTOL, 1e-5, "dseg")
    for k, v in st.items():
        if ("grad:" + k) in a:
            assert_close(v.grad, a["grad:" + k], 2e-4, 1e-5, "d" + k)
        if ("after:" + k) in a:          # u, v, running stats, num_batches_tracked
            assert_close(v, a["after:" + k], RTOL, 1e-6, "state " + k)
    with torch.no_grad():
        y_eval = oracle.spade_resblock(st, "", a["x"], a["seg"], training=False)
    assert_close(y_eval, a["y_eval"], RTOL, 1e-5, "eval out")


def test_syncbn_multi_replica_formula():
    _, a = load_golden("syncbn")
    rm, rv = torch.zeros(5), torch.ones(5)
    ys = oracle.syncbn_multi_replica([a["x0"], a["x1"]], rm, rv)
    assert_close(ys[0], a["y0"], RTOL, 1e-6)
    assert_close(ys[1], a["y1"], RTOL, 1e-6)
    assert_close(rm, a["running_mean"], RTOL, 1e-6)
    assert_close(rv, a["running_var"], RTOL, 1e-6)


def _train_fixture():
    meta, a = load_golden("train_step")
    vocab = make_vocab(meta["vocab"])
    opt = make_opt(vocab, meta["argv"])
    sg = state_from_shapes(meta["shapes"]["sg"], seed=11)
    w = sg["trans_candidates_weights"]
    for k in list(sg):
        if k.endswith("predicates_transitive_weights"):
            sg[k] = w
    g, d = state_from_shapes(meta["shapes"]["g"], seed=12), state_from_shapes(meta["shapes"]["d"], seed=13)
    batch = (a["imgs"], a["objs"], a["boxes"], a["triplets"], None, a["tt"], None, None)
    return meta, a, opt, sg, g, d, batch


def _check_image(imgs_pred, fresh_ts, batch, a, fixture, msg):
    """The generated image of a train-step fixture against the reference's.

    Two fp32 evaluations of the generator agree to ~1e-5 only when they round alike: the fixture's fp32 image was made on
    one CPU, and the same oracle on another instruction set or thread count lands 4-6e-5 from it (train_step_masks: both
    fp32 images sit 1.8e-4 from the exact one).  So the algorithm is judged in float64, against the reference's own
    generator evaluated in float64 on the fixture's weights and batch (step_images_fp64.npz, measured 4e-14 apart), and
    the oracle's fp32 arithmetic against that exact image: at most 3x the reference's own fp32 distance from it, in
    relative L2 and in max norm (the factor of tests/fp64_band.py; measured <= 1.44 over oneDNN ISAs and thread counts).
    `fresh_ts`: the fixture's state before the step, rebuilt (the fp64 forward advances its integer BatchNorm counters)."""
    from fp64_band import errors
    img64 = generated_image64(fresh_ts, batch)
    ref64 = load_golden("step_images_fp64")[1][fixture]
    assert_close(img64, ref64, 1e-9, 1e-11, msg + " (fp64 oracle vs fp64 reference)")
    (o_l2, o_max), (r_l2, r_max) = errors(imgs_pred, ref64), errors(a["imgs_pred"], ref64)
    assert o_l2 <= 3 * r_l2 and o_max <= 3 * r_max, "%s: fp32 oracle l2 %.2e max %.2e from fp64, fp32 reference %.2e %.2e" % (
        msg, o_l2, o_max, r_l2, r_max)


def test_full_train_step_matches_reference():
    meta, a, opt, sg, g, d, batch = _train_fixture()
    ts = oracle.TrainState(opt, sg, g, d)
    G, D, imgs_pred = oracle.train_step(ts, batch)
    _check_image(imgs_pred, oracle.TrainState(opt, *_train_fixture()[3:6]), batch, a, "train_step", "imgs_pred")
    for k in ("bbox_pred_all", "bbox_pred", "GAN_Img", "GAN_Feat", "total_loss"):
        assert_close(G[k].reshape(a["G:" + k].shape), a["G:" + k], RTOL, 1e-5, "G " + k)
    for k in ("D_img_fake", "D_img_real", "total_img_loss"):
        assert_close(D[k].reshape(a["D:" + k].shape), a["D:" + k], RTOL, 1e-5, "D " + k)
    # Post-step state.  Buffers (u, v, running stats) are compared tightly.  Parameters moved by
    # Adam's first step, lr*g/(|g|+1e-8): where the true gradient is zero (e.g. a conv bias that a
    # BatchNorm removes) the sign of rounding noise decides a +-lr move, so elements are compared
    # tightly only where the reference gradient is non-negligible, and within 2.2*lr elsewhere.
    lr = opt.learning_rate

    def check_param(name, mine, want, gkey):
        if gkey in a:
            g = a[gkey]
            sig = g.abs() > 1e-5 * g.abs().max().clamp_min(1e-30)
            assert_close(mine.detach()[sig], want[sig], 1e-3, 2e-6, name)
        assert_close(mine, want, 0, 2.2 * max(lr, 1e-2 if "trans" in name or "transitive" in name else lr), name)

    for k, v in a.items():
        if k.startswith("sg_after:"):
            check_param(k, sg[k[9:]], v, "sggrad:" + k[9:])
        elif k.startswith("d_after:"):
            name = k[8:]
            if any(b in name for b in ("weight_u", "weight_v")):
                assert_close(d[name], v, 1e-3, 2e-6, k)
            else:
                check_param(k, d[name], v, "dgrad:" + name)
        elif k.startswith("g_after:"):
            name = k[8:]
            if any(b in name for b in ("running_", "weight_u", "weight_v", "num_batches")):
                assert_close(g[name], v, 1e-3, 2e-6, k)
            else:
                check_param(k, g[name], v, "ggrad:" + name)
    for k, v in a.items():
        if k.startswith("ggrad:"):
            assert_close(g[k[6:]].grad, v, 1e-3, 1e-6, k)
        if k.startswith("sggrad:") and sg[k[7:]].grad is not None:
            assert_close(sg[k[7:]].grad, v, 1e-3, 1e-6, k)
    # D gradients of the D step
    n = 0
    for k, v in a.items():
        if k.startswith("dgrad:"):
            assert_close(d[k[6:]].grad, v, 1e-3, 1e-6, k)
            n += 1
    assert n >= 10


def test_discriminator_features_eval():
    meta, a, opt, sg, g, d, batch = _train_fixture()
    d_after = sub_state(a, "d_after:", requires_grad=False)
    with torch.no_grad():
        feats = oracle.multiscale_discriminator(d_after, opt.vocab, opt.image_size[0], batch[0], batch[1], batch[2],
                                                training=False)
    for i, scale in enumerate(feats):
        for j, f in enumerate(scale):
            assert_close(f, a["dfeat_%d_%d" % (i, j)], RTOL, 1e-5, "dfeat %d %d" % (i, j))


def test_masks_to_layout():
    meta, a = load_golden("masks_layout")
    for H in meta["sizes"]:
        for tag, key in (("int", "masks"), ("soft", "soft")):
            vecs = a["vecs"].clone().requires_grad_(True)
            out = oracle.masks_to_layout(vecs, a["boxes"], a[key], H, H)
            assert_close(out, a["out_%s_%d" % (tag, H)], RTOL, ATOL, "masks layout %s %d" % (tag, H))
            (gv,) = torch.autograd.grad((out * a["w_%s_%d" % (tag, H)]).sum(), [vecs])
            assert_close(gv, a["gvecs_%s_%d" % (tag, H)], RTOL, 1e-5, "masks layout dvecs %s %d" % (tag, H))


def test_row_gap_fixtures():
    """Painter's compositing (`test_mode`), box gradients of the masks layout, non-square sizes,
    build_mlp(batch_norm='batch') and the affine SynchronizedBatchNorm2d — oracle vs the reference's outputs."""
    meta, a = load_golden("row_gaps")
    for (H, W) in ((32, 32), (24, 40)):
        for tag, key in (("bin", "p_bin"), ("soft", "p_soft")):
            out = oracle.masks_to_layout(a["p_vecs"], a["p_boxes"], a[key], H, W, test_mode=True)
            assert_close(out, a["paint_%s_%dx%d" % (tag, H, W)], RTOL, ATOL, "paint %s %dx%d" % (tag, H, W))
        vecs = a["p_vecs"].clone().requires_grad_(True)
        boxes = a["p_boxes"].clone().requires_grad_(True)
        out = oracle.masks_to_layout(vecs, boxes, a["p_soft"], H, W)
        t = "%dx%d" % (H, W)
        assert_close(out, a["m_out_" + t], RTOL, ATOL, "masks layout " + t)
        gv, gb = torch.autograd.grad((out * a["m_w_" + t]).sum(), [vecs, boxes])
        assert_close(gv, a["m_gvecs_" + t], RTOL, 1e-5, "masks layout dvecs " + t)
        assert_close(gb, a["m_gboxes_" + t], RTOL, 1e-5 * float(a["m_gboxes_" + t].abs().max()), "masks layout dboxes " + t)
    st = state_from_shapes(meta["mlp_shapes"], seed=62)  # the state the fixture was generated from
    x = a["mlp_x"].clone().requires_grad_(True)
    y = oracle.mlp2_batchnorm(st, "", x, True)
    assert_close(y, a["mlp_y"], RTOL, ATOL, "mlp(batch) y")
    (y * a["mlp_w"]).sum().backward()
    assert_close(x.grad, a["mlp_gx"], RTOL, 1e-5, "mlp(batch) dx")
    for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias"):
        g = a["mlp_grad:" + k]
        if float(g.abs().max()) < 1e-6:                  # Linear bias in front of BatchNorm: analytically zero
            assert float(st[k].grad.abs().max()) < 1e-5
        else:
            assert_close(st[k].grad, g, RTOL, 1e-5, "mlp(batch) d" + k)
    for k in ("1.running_mean", "1.running_var", "1.num_batches_tracked"):
        assert_close(st[k], a["mlp_after:" + k], RTOL, 1e-6, "mlp(batch) " + k)
    with torch.no_grad():
        assert_close(oracle.mlp2_batchnorm(st, "", a["mlp_x"], False), a["mlp_y_eval"], RTOL, ATOL, "mlp(batch) eval")
    bn = {"weight": a["bn_weight"].clone().requires_grad_(True), "bias": a["bn_bias"].clone().requires_grad_(True),
          "running_mean": torch.zeros(8), "running_var": torch.ones(8)}
    xb = a["bn_x"].clone().requires_grad_(True)
    yb = oracle.syncbn_affine_single_device(bn, "", xb, True)
    assert_close(yb, a["bn_y"], RTOL, ATOL, "affine syncbn y")
    (yb * a["bn_w"]).sum().backward()
    assert_close(xb.grad, a["bn_gx"], RTOL, 1e-5, "affine syncbn dx")
    assert_close(bn["weight"].grad, a["bn_gweight"], RTOL, 1e-5, "affine syncbn dweight")
    assert_close(bn["bias"].grad, a["bn_gbias"], RTOL, 1e-5, "affine syncbn dbias")
    assert_close(bn["running_mean"], a["bn_running_mean"], RTOL, 1e-6, "affine syncbn running_mean")
    assert_close(bn["running_var"], a["bn_running_var"], RTOL, 1e-6, "affine syncbn running_var")
    with torch.no_grad():
        assert_close(oracle.syncbn_affine_single_device(bn, "", a["bn_x"], False), a["bn_y_eval"], RTOL, ATOL, "eval")


def test_row_gap_r3_fixtures():
    """Gradients w.r.t. the masks (and boxes) of masks_to_layout and w.r.t. the boxes of the object crops — oracle vs
    the reference's autograd outputs."""
    meta, a = load_golden("row_gaps_r3")
    for M in meta["mask_sizes"]:
        for (H, W) in meta["sizes"]:
            t = "%d_%dx%d" % (M, H, W)
            vecs, boxes, soft = [a[k].clone().requires_grad_(True) for k in ("vecs", "boxes", "soft_%d" % M)]
            out = oracle.masks_to_layout(vecs, boxes, soft, H, W)
            assert_close(out, a["out_" + t], RTOL, ATOL, "masks layout " + t)
            gv, gb, gm = torch.autograd.grad((out * a["w_" + t]).sum(), [vecs, boxes, soft])
            assert_close(gv, a["gvecs_" + t], RTOL, 1e-5, "dvecs " + t)
            assert_close(gb, a["gboxes_" + t], RTOL, 1e-5 * float(a["gboxes_" + t].abs().max()), "dboxes " + t)
            assert_close(gm, a["gmasks_" + t], RTOL, 1e-5, "dmasks " + t)
    vocab = make_vocab(meta["vocab"])
    imgs, cb = a["c_imgs"].clone().requires_grad_(True), a["c_boxes"].clone().requires_grad_(True)
    crops, _ = oracle.crop_objects(imgs, a["c_objs"], cb, vocab, meta["crop_size"])
    assert_close(crops, a["c_crops"], RTOL, ATOL, "crops")
    gi, gcb = torch.autograd.grad((crops * a["c_w"]).sum(), [imgs, cb])
    assert_close(gi, a["c_gimgs"], RTOL, 1e-5, "d imgs")
    assert_close(gcb, a["c_gboxes"], RTOL, 1e-5 * float(a["c_gboxes"].abs().max()), "d crop boxes")


def test_object_crops():
    meta, a = load_golden("crops")
    vocab = make_vocab(meta["vocab"])
    imgs = a["imgs"].clone().requires_grad_(True)
    crops, labels = oracle.crop_objects(imgs, a["objs"], a["boxes"], vocab, meta["size"])
    assert_close(crops, a["crops"], RTOL, ATOL, "crops")
    (gi,) = torch.autograd.grad((crops * a["w"]).sum(), [imgs])
    assert_close(gi, a["gimgs"], RTOL, 1e-5, "d imgs")
    want = torch.cat([a["objs"][b][oracle.remove_dummy_objects(a["objs"][b], vocab)][:, 0] for b in range(3)])
    assert torch.equal(labels, want)


def _objdisc_fixture():
    meta, a = load_golden("train_step_objdisc")
    vocab = make_vocab(meta["vocab"])
    opt = make_opt(vocab, meta["argv"])
    sh = meta["shapes"]
    sg = state_from_shapes(sh["sg"], seed=21)
    w = sg["trans_candidates_weights"]
    for k in list(sg):
        if k.endswith("predicates_transitive_weights"):
            sg[k] = w
    g, d = state_from_shapes(sh["g"], seed=22), state_from_shapes(sh["d"], seed=23)
    dobj = state_from_shapes(sh["dobj"], seed=24)
    batch = (a["imgs"], a["objs"], a["boxes"], a["triplets"], None, a["tt"], None, None)
    return meta, a, opt, sg, g, d, dobj, batch


def test_default_train_step_with_object_discriminator():
    """use_img_disc=0 (the reference's default recipe): image + object discriminators."""
    meta, a, opt, sg, g, d, dobj, batch = _objdisc_fixture()
    ts = oracle.TrainState(opt, sg, g, d, dobj)
    G, D, _ = oracle.train_step(ts, batch)
    for k in ("bbox_pred", "GAN_Img", "GAN_Feat", "GAN_Obj", "GAN_Ac", "total_loss"):
        assert_close(G[k].reshape(a["G:" + k].shape), a["G:" + k], RTOL, 1e-5, "G " + k)
    for k in ("D_img_fake", "D_img_real", "total_img_loss", "D_img_wrong", "D_obj", "D_ac_real", "D_ac_fake",
              "total_obj_loss"):
        assert_close(D[k].reshape(a["D:" + k].shape), a["D:" + k], RTOL, 1e-5, "D " + k)
    for k, v in a.items():
        if k.startswith("ograd:"):
            assert_close(dobj[k[6:]].grad, v, 1e-3, 1e-6, k)
        elif k.startswith("ggrad:"):
            assert_close(g[k[6:]].grad, v, 1e-3, 1e-6, k)
        elif k.startswith("d_after:"):
            assert_close(d[k[8:]], v, 1e-3, 2e-6, k)             # u after FIVE power iterations
        elif k.startswith("o_after:") and ("running_" in k or "num_batches" in k):
            assert_close(dobj[k[8:]], v, 1e-3, 2e-6, k)


def test_vgg_loss():
    """VGG19 slices + VGGLoss (loss.py:102-117) on the seeded weights the fixture was made with."""
    meta, a = load_golden("vgg_loss")
    st = state_from_shapes(meta["shapes"], seed=31, requires_grad=False)
    x = a["x"].clone().requires_grad_(True)
    feats = oracle.vgg19_features(st, x)
    assert len(feats) == 5
    for i, f in enumerate(feats):
        assert_close(f.abs().mean(), a["feat_abs_mean_%d" % i], RTOL, ATOL, "vgg feat mean %d" % i)
        if i >= 2:
            assert_close(f, a["feat_%d" % i], RTOL, 1e-5, "vgg feat %d" % i)
    loss = oracle.vgg_loss(st, x, a["y"])
    assert_close(loss, a["loss"], RTOL, ATOL, "vgg loss")
    loss.backward()
    assert_close(x.grad, a["grad_x"], RTOL, 1e-6, "vgg dx")


def _masks_fixture():
    meta, a = load_golden("train_step_masks")
    vocab = make_vocab(meta["vocab"])
    opt = make_opt(vocab, meta["argv"])
    sh = meta["shapes"]
    sg = state_from_shapes(sh["sg"], seed=41)
    w = sg["trans_candidates_weights"]
    for k in list(sg):
        if k.endswith("predicates_transitive_weights"):
            sg[k] = w
    g, d = state_from_shapes(sh["g"], seed=42), state_from_shapes(sh["d"], seed=43)
    dobj, dmask = state_from_shapes(sh["dobj"], seed=44), state_from_shapes(sh["dmask"], seed=45)
    batch = (a["imgs"], a["objs"], a["boxes"], a["triplets"], None, a["tt"], a["masks"], None)
    return meta, a, opt, sg, g, d, dobj, dmask, batch


def test_train_step_with_masks():
    """--mask_size 8: mask net (incl. its BatchNorm over padded slots), masks layout in G and D, mask BCE,
    mask discriminator G/D terms and its optimiser step, against the reference."""
    meta, a, opt, sg, g, d, dobj, dmask, batch = _masks_fixture()
    assert opt.mask_size == 8
    _, _, masks_pred = oracle.sg2layout_forward({k: v.detach().clone() for k, v in sg.items()}, opt.vocab, batch[1],
                                                batch[3], batch[5], mask_noise=a["mask_noise"])
    assert_close(masks_pred, a["masks_pred"], RTOL, 1e-6, "masks_pred")
    ts = oracle.TrainState(opt, sg, g, d, dobj, None, dmask, a["mask_noise"])
    G, D, imgs_pred = oracle.train_step(ts, batch)
    sg0, g0, d0, dobj0, dmask0 = _masks_fixture()[3:8]
    _check_image(imgs_pred, oracle.TrainState(opt, sg0, g0, d0, dobj0, None, dmask0, a["mask_noise"]), batch, a,
                 "train_step_masks", "imgs_pred (masks layout)")
    assert {k[2:] for k in a if k.startswith("G:")} == set(G.keys())
    assert {k[2:] for k in a if k.startswith("D:")} == set(D.keys())
    for k in G:
        assert_close(G[k].reshape(a["G:" + k].shape), a["G:" + k], RTOL, 1e-5, "G " + k)
    for k in D:
        assert_close(D[k].reshape(a["D:" + k].shape), a["D:" + k], RTOL, 1e-5, "D " + k)
    n = 0
    for k, v in a.items():
        if k.startswith("mgrad:"):
            assert_close(dmask[k[6:]].grad, v, 1e-3, 1e-6 + 1e-3 * float(v.abs().max()), k)
            n += 1
        elif k.startswith("sggrad:"):
            assert_close(sg[k[7:]].grad, v, 1e-3, 1e-7 + 1e-3 * float(v.abs().max()), k)
            n += 1
        elif k.startswith("sg_after:"):
            assert_close(sg[k[9:]], v, 1e-3, 2e-6, k)
            n += 1
    assert n > 15


def test_converse_reinforce_signal():
    """--learned_converse (scripts/train.py:370-378): log-probability of the sampled converse edges and the
    REINFORCE loss / gradient, oracle and product helpers against the reference's own functions."""
    from canonicalsg2im_amd.scripts import graphs_utils as product
    meta, a = load_golden("converse")
    vocab = make_vocab(meta["vocab"])
    w = a["w"].clone().requires_grad_(True)
    loss = oracle.converse_loss(w, vocab, a["r"], a["counts"])
    assert_close(loss, a["loss"], RTOL, 1e-6, "loss_conv")
    loss.backward()
    assert_close(w.grad, a["grad_w"], RTOL, 1e-6, "d converse weights")
    non_meta = sorted(set(vocab["pred_name_to_idx"].values()) - {0, 1})
    triu = torch.triu(a["w"], diagonal=0)
    assert_close(product.calc_log_p(triu + triu.t(), non_meta, a["counts"]), a["log_prob"], RTOL, 1e-5, "log_prob")
    assert_close(oracle.calc_log_p(triu + triu.t(), non_meta, a["counts"]), a["log_prob"], RTOL, 1e-5, "log_prob (oracle)")
