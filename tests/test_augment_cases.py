"""The restatement of DiffAugment (tests/augment_cases.py) against fixed vectors, against the host half of the shared header
(through the ABI's host entry), against itself (the backward is the adjoint of the forward) and against hand-made maps; the
coverage of the case table the device is held to (tests/test_gpu_augment.py); the flags and what the Python layer refuses.
CPU only."""
import numpy as np
import pytest
import torch

import augment_cases as ac


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import ops
    return ops


def test_hash_equals_its_fixed_vectors():
    assert ac.step_py(0, 0) == 0xe220a8397b1dcdaf                # splitmix64's first output from state 0, as published
    for key, (h, g1) in ac.HASH_VECTORS:
        assert ac.key_py(*key) == h and ac.step_py(h, 1) == g1
        assert int(ac.step_np(np.uint64(h), np.uint64(1))) == g1
    seed, it, p, rank, H = ac.ROW_VECTORS_KEY
    assert [ac.row_py(seed, it, p, rank, n, H) for n in range(3)] == ac.ROW_VECTORS
    assert ac.table_np(seed, it, p, rank, 3, H).tolist() == ac.ROW_VECTORS
    # the row index is the low word and the rank the high word of ONE key word
    assert ac.key_py(1, 2, 3, 1, 0) == ac.step_py(ac.step_py(ac.step_py(ac.step_py(0, 1), 2), 3), 1 << 32)


def test_host_half_of_the_header_gives_the_restatements_words(ops):
    for seed, it, p, rank, H, rows in ((0, 0, 0, 0, 2, 5), (7, 3, 2, 1, 256, 64), (99, 1000, 5, 0, 33, 300),
                                       ((1 << 64) - 1, (1 << 63) - 1, 4, (1 << 31) - 1, 16, 10), (5, 1, 3, 0, 32, 1)):
        got = ops.augment_table_host(seed, it, p, rows, H, rank=rank).numpy()
        assert got.dtype == np.int32 and np.array_equal(got, ac.table_np(seed, it, p, rank, rows, H)), (seed, it, p, rank, H)
    assert ops.augment_table_host(1, 1, 1, 0, 8).shape == (0, 8)
    for bad, what in ((dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(iteration=-1), "iteration"),
                      (dict(pass_id=1 << 31), "pass_id"), (dict(rank=-1), "rank"), (dict(rows=-1), "rows"), (dict(H=1), "H"),
                      (dict(H=2.0), "H")):
        with pytest.raises(RuntimeError, match=what):
            ops.augment_table_host(**dict(dict(seed=0, iteration=0, pass_id=0, rows=1, H=8), **bad))


@pytest.mark.parametrize("H", [2, 7, 8, 32, 33, 256])
def test_every_draw_reaches_both_ends_of_its_range(H):
    t, size, centres = ac.extents(H)
    assert (t, size) == (int(H * 0.125 + 0.5), int(H * 0.5 + 0.5)) and centres == H + (1 - size % 2)
    tab = np.concatenate([ac.table_np(3, it, p, r, 2000, H) for it, p, r in ((0, 0, 0), (1, 2, 0), (7, 5, 1))])
    b, s, c = (tab[:, k].view(np.float32) for k in range(3))
    assert -0.5 <= b.min() < -0.49 and 0.49 < b.max() < 0.5
    assert 0.0 <= s.min() < 0.02 and 1.98 < s.max() < 2.0
    assert 0.5 <= c.min() < 0.51 and 1.49 < c.max() <= 1.5
    for k in (3, 4):
        assert tab[:, k].min() == -t and tab[:, k].max() == t
    for k in (5, 6):
        centre = tab[:, k] + size // 2
        assert centre.min() == 0 and centre.max() == centres - 1          # with an even size the centre reaches H
    if size % 2 == 0:
        assert (tab[:, 5] + size // 2 == H).any()
    assert (tab[:, 7] == size).all()
    if H == 2:
        assert t == 0 and (tab[:, 3:5] == 0).all()                         # translation is the identity
    # a draw does not move when another policy is switched: the rows do not depend on a policy at all, and the keys differ
    assert not np.array_equal(ac.table_np(3, 0, 0, 0, 8, H)[:, :3], ac.table_np(3, 0, 1, 0, 8, H)[:, :3])
    assert not np.array_equal(ac.table_np(3, 0, 0, 0, 8, H)[:, :3], ac.table_np(3, 0, 0, 1, 8, H)[:, :3])
    assert not np.array_equal(ac.table_np(3, 0, 0, 0, 8, H)[:, :3], ac.table_np(4, 0, 0, 0, 8, H)[:, :3])


def _rows_for(shape, k=0):
    rows = ac.boundary_rows(shape[1])
    return np.stack([rows[(k + n) % len(rows)] for n in range(shape[0])])


@pytest.mark.parametrize("policy", ac.ALL_POLICIES)
def test_backward_restatement_is_the_adjoint_of_the_forward(policy):
    """<fwd(x) - fwd(0), g> = <x, bwd(g)> to 1e-12 relative: brightness makes the map affine, x -> A x + fwd(0), and the
    backward is the adjoint of A.  With b = 0 (rows of the second loop) fwd(0) = 0 and the identity holds as it stands."""
    rng = np.random.default_rng(policy)
    for shape in ac.SHAPES:
        N, H, Ct, c0 = shape
        for k in range(0, 9, 2):
            table = _rows_for(shape, k)
            x = rng.standard_normal((N, H, H, Ct)).astype(np.float32)
            g = rng.standard_normal((N, H, H, Ct)).astype(np.float32)
            y, _, _ = ac.restate_fwd(x, table, c0, policy)
            y0, _, _ = ac.restate_fwd(np.zeros_like(x), table, c0, policy)
            gx, _, _ = ac.restate_bwd(g, table, c0, policy)
            lhs, rhs = ((y - y0) * g).sum(), (x.astype(np.float64) * gx).sum()
            scale = np.abs((y - y0) * g).sum() + np.abs(x * gx).sum() + 1e-300
            assert abs(lhs - rhs) <= 1e-12 * scale, (shape, k, lhs, rhs)
            zero_b = table.copy()
            zero_b[:, 0] = 0
            y, _, _ = ac.restate_fwd(x, zero_b, c0, policy)
            gx, _, _ = ac.restate_bwd(g, zero_b, c0, policy)
            lhs, rhs = (y * g).sum(), (x.astype(np.float64) * gx).sum()
            assert abs(lhs - rhs) <= 1e-12 * (np.abs(y * g).sum() + np.abs(x * gx).sum() + 1e-300), (shape, k)


def test_restatement_on_hand_made_maps():
    H, Ct, c0 = 4, 4, 0
    x = np.arange(H * H * Ct, dtype=np.float32).reshape(1, H, H, Ct) + 1.0
    # translation: out[y, x] = in[y - ty, x - tx], zero outside
    row = ac.make_row(0.0, 1.0, 1.0, 1, -1, 0, 0, 0)[None]
    y, exact, _ = ac.restate_fwd(x, row, c0, ac.TRANSLATION)
    assert exact.all() and (y[0, 3] == 0).all() and (y[0, :, 0] == 0).all()
    assert np.array_equal(y[0, 0, 1], x[0, 1, 0]) and np.array_equal(y[0, 2, 3], x[0, 3, 2])
    # cutout: rows [y0, y0 + size) x columns [x0, x0 + size), clipped by the map
    row = ac.make_row(0.0, 1.0, 1.0, 0, 0, -1, 2, 2)[None]
    y, exact, _ = ac.restate_fwd(x, row, c0, ac.CUTOUT)
    cut = np.zeros((H, H), bool)
    cut[0:1, 2:4] = True
    assert exact.all() and (y[0][cut] == 0).all() and np.array_equal(y[0][~cut], x[0][~cut].astype(np.float64))
    # the cutout is applied after the translation: it is not shifted
    row = ac.make_row(0.0, 1.0, 1.0, 1, 1, -1, 2, 2)[None]
    y, _, _ = ac.restate_fwd(x, row, c0, ac.TRANSLATION | ac.CUTOUT)
    assert (y[0][cut] == 0).all() and np.array_equal(y[0, 1, 1], x[0, 0, 0])
    # colour by hand on one pixel row repeated: x = (1, 2, 6) everywhere, b = 0.5, s = 0, c = 0.5
    x = np.tile(np.asarray([1, 2, 6, 9], np.float32), (1, H, H, 1))
    row = ac.make_row(0.5, 0.0, 0.5, 0, 0, 0, 0, 0)[None]
    y, exact, L = ac.restate_fwd(x, row, c0, ac.COLOR)
    assert np.allclose(y[0, ..., :3], 3.5) and (y[0, ..., 3] == 9).all()        # s = 0: the pixel mean 3.5; mu = 3.5 too
    assert exact[0, ..., 3].all() and not exact[0, ..., :3].any() and L[0] == 10.5       # t = 1.5 + 2.5 + 6.5
    row = ac.make_row(0.0, 2.0, 1.0, 0, 0, 0, 0, 0)[None]
    y, _, _ = ac.restate_fwd(x, row, c0, ac.COLOR)
    assert np.allclose(y[0, 0, 0, :3], [-1.0, 1.0, 9.0])                         # (x - 3) * 2 + 3
    # a policy that is off leaves its part alone
    full = ac.make_row(0.25, 0.5, 1.25, 1, 1, 0, 0, 2)[None]
    y, exact, _ = ac.restate_fwd(x, full, c0, ac.COLOR)
    assert np.array_equal(y[0, ..., 3], x[0, ..., 3].astype(np.float64)) and exact[0, ..., 3].all()
    y, exact, _ = ac.restate_fwd(x, full, c0, ac.TRANSLATION | ac.CUTOUT)
    assert exact.all() and set(np.unique(y[0, ..., :3])) <= {0.0, 1.0, 2.0, 6.0}


def test_case_table_covers_what_it_says():
    assert ac.SHAPES == [(1, 2, 4, 0), (3, 4, 4, 0), (2, 8, 8, 4), (2, 8, 8, 5), (3, 16, 12, 8), (2, 32, 40, 32)]
    assert len(ac.ALL_POLICIES) == 7
    for N, H, Ct, c0 in ac.SHAPES + ac.SPLIT_SHAPES:
        assert Ct % 4 == 0 and c0 + 3 <= Ct and H >= 2
        rows = ac.boundary_rows(H)
        t, size, centres = ac.extents(H)
        assert {(r[3], r[4]) for r in rows.tolist()} == {(a, b) for a in (-t, 0, t) for b in (-t, 0, t)}
        cy, cx = rows[:, 5] + size // 2, rows[:, 6] + size // 2
        assert {0, centres - 1, centres // 2} == set(cy.tolist()) == set(cx.tolist())
        bsc = rows[:, :3].view(np.float32)
        assert (bsc[:, 1] == 0).any() and (bsc[:, 2] == 0.5).any() and (bsc[:, 0] == -0.5).any()
    # either side of every point where the reduction takes another path (the launch rule in the module docstring)
    rule = {s: ac.launch_rule(s[0], s[1]) for s in ac.SPLIT_SHAPES}
    assert rule[(2, 16, 4, 0)][0] == 1 and rule[(2, 17, 4, 0)][0] == 2
    assert rule[(1, 256, 4, 0)][2] == 1 and rule[(1, 257, 4, 1)][2] == 2
    assert rule[(8, 256, 4, 0)][1] == 8 * 256 == ac.MAX_GRID and 9 * 256 > ac.MAX_GRID == rule[(9, 256, 4, 0)][1]
    assert all(ac.launch_rule(H=H, N=1)[0] == 1 for H in range(2, 17)) and ac.launch_rule(1, 17)[0] == 2
    assert max(ac.launch_rule(1, H)[2] for H in range(2, 257)) == 1


def test_launch_rule_is_the_librarys(ops):
    from canonicalsg2im_amd._lib import lib
    assert ops.AUG_CHUNK == ac.CHUNK
    for N, H, _, _ in ac.SHAPES + ac.SPLIT_SHAPES:
        assert lib.csg_augment_workspace_bytes(N, H) == ac.workspace_bytes(N, H)
    assert lib.csg_augment_workspace_bytes(1, 1) == -1


def test_the_python_layer_refuses_by_the_arguments_name(ops):
    """Every refusal below is raised on the host, before a device pointer is asked for: the tensors are CPU tensors."""
    x = ops.empty_nhwc(2, 8, 4, 4, "cpu", zero=True)
    table = torch.zeros((2, 8), dtype=torch.int32)
    for args, what in (((ops.empty_nhwc(2, 6, 4, 4, "cpu"), table, 0, 7), "Ct % 4 != 0"),
                       ((x, table, 6, 7), "c0 \\+ 3 > Ct"), ((x, table, -1, 7), "c0 \\+ 3 > Ct"),
                       ((ops.empty_nhwc(2, 8, 1, 1, "cpu"), table, 0, 7), "H < 2"),
                       ((x, table[:1], 0, 7), "fewer than N = 2"), ((x, table.long(), 0, 7), "int32 \\(rows, 8\\)"),
                       ((x, torch.zeros((2, 4), dtype=torch.int32), 0, 7), "int32 \\(rows, 8\\)"),
                       ((ops.empty_nhwc(2, 8, 4, 6, "cpu"), table, 0, 7), "\\(N, Ct, H, H\\)"),
                       ((x.double(), table, 0, 7), "fp32"), ((x, table, 5, 7), "no CPU path")):
        with pytest.raises(RuntimeError, match=what):
            ops.d_augment(*args)
    for bad in (8, -1, "color", None, True):
        with pytest.raises(RuntimeError, match="policy must be a mask"):
            ops.d_augment(x, table, 5, bad)
    from canonicalsg2im_amd.d_augment import policy_mask, policy_names
    for bad in ("colour", "color,flip", "color;cutout", "color,", 5, ["cutout"]):
        with pytest.raises(ValueError, match="d_augment"):
            policy_mask(bad)
    assert [policy_mask(p) for p in ("", None, "color", "cutout,color", "color, translation ,cutout")] == [0, 0, 1, 5, 7]
    assert (ops.AUG_COLOR, ops.AUG_TRANSLATION, ops.AUG_CUTOUT) == (1, 2, 4) and policy_names(6) == "translation,cutout"


def test_flags(capsys):
    from canonicalsg2im_amd.scripts import train
    a = train.build_parser().parse_args([])
    assert a.d_augment == "" and a.d_augment_seed == 0
    a = train.build_parser().parse_args(["--d_augment", "cutout,color", "--d_augment_seed", "12"])
    assert a.d_augment == "color,cutout" and a.d_augment_seed == 12
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train.main(["--d_augment", "colour"])
    err = capsys.readouterr().err
    assert "unknown policy 'colour'" in err and "color,translation,cutout" in err, err
    for bad in (["--d_augment", "color,flip"], ["--d_augment_seed", "-1"], ["--d_augment_seed", "x"]):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train.main(["--help"])
    out = capsys.readouterr().out
    assert "--d_augment POLICIES" in out and "--d_augment_seed N" in out


def test_off_is_off_on_the_host(ops):
    """No flag, an empty flag, or a namespace from before the flags: no DAugment object, today's checkpoint keys, and the
    discriminators' class attribute stays None.  With the flag the object holds what the checkpoint will carry."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.d_augment import DAugment
    from canonicalsg2im_amd.synth import make_vocab
    tiny = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
            "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2"]
    keys = None
    for strip in (True, False):
        opt = T.make_opt(make_vocab("tiny"), tiny)
        if strip:
            del opt.d_augment, opt.d_augment_seed
        torch.manual_seed(0)
        tr = T.Trainer(opt, torch.device("cpu"))
        assert tr.d_augment is None and tr.discriminator.img_discriminator.d_augment is None
        assert tr.discriminator.obj_discriminator.d_augment is None
        keys = set(tr.checkpoint_dict())
        assert "d_augment" not in keys
    tr = T.Trainer(T.make_opt(make_vocab("tiny"), tiny + ["--d_augment", "cutout,translation", "--d_augment_seed", "9"]),
                   torch.device("cpu"))
    assert isinstance(tr.d_augment, DAugment) and tr.discriminator.obj_discriminator.d_augment is tr.d_augment
    ck = tr.checkpoint_dict()
    assert set(ck) == keys | {"d_augment"} and ck["d_augment"] == {"seed": 9, "iteration": 0, "policies": "translation,cutout"}
    said = []
    tr.d_augment.load_meta({"seed": 9, "iteration": 5, "policies": "translation,cutout"}, say=said.append)
    assert tr.d_augment.iteration == 5 and not said
    tr.d_augment.load_meta({"seed": 1, "iteration": 7, "policies": "color"}, say=said.append)
    assert tr.d_augment.iteration == 7 and len(said) == 1 and "'color'" in said[0] and "'translation,cutout'" in said[0]
    tr.d_augment.load_meta(None, say=said.append)
    assert tr.d_augment.iteration == 0 and len(said) == 1
    with pytest.raises(ValueError, match="unknown policy"):
        T.Trainer(T.make_opt(make_vocab("tiny"), tiny, d_augment="colour"), torch.device("cpu"))
