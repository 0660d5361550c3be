"""The input stage's host restatements against the libraries they restate (CPU; tests/preprocess_cases.py)."""
import numpy as np
import pytest
import torch

import preprocess_cases as pc


@pytest.mark.parametrize("case", pc.CASES + pc.LIMIT_CASES, ids=pc.case_id)
def test_pil_resize_u8_is_pillows_bilinear_resize_byte_for_byte(case):
    """Every row of the table, the 251-tap one included: 0 differing bytes against the installed Pillow."""
    Image = pytest.importorskip("PIL.Image")
    h, w, H, W = case[:4]
    img = pc.case_image(case)
    want = np.asarray(Image.fromarray(img, "RGB").resize((W, H), Image.BILINEAR))
    got = pc.pil_resize_u8(img, H, W)
    differing = int((want != got).sum())
    print("%s: %d differing bytes of %d" % (pc.case_id(case), differing, want.size))
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    assert differing == 0


def test_the_table_holds_one_row_beyond_the_device_range():
    unsupported = [c for c in pc.CASES if not pc.supported(*c[:4])]
    assert [c[:4] for c in unsupported] == [(17, 1000, 8, 8)]
    assert len(pc.CASES) == 8
    assert all(pc.supported(*c[:4]) for c in pc.LIMIT_CASES)
    taps = [len(k) for c in pc.LIMIT_CASES for _, k in pc.axis_coefficients(c[0], c[2])]
    # int(c + fs + 0.5) - int(c - fs + 0.5) is at most 2 * fs for an integer fs: Pillow's table width 2 * ceil(fs) + 1 = 129
    # is an allocation bound, 128 taps is the most a supported size produces, and a row of the list reaches it
    assert max(taps) == 2 * pc.MAX_FILTERSCALE


def test_to_float_against_the_float64_formula():
    """All 256 byte values x 3 channels.  The three fp32 operations round three times where the float64 formula rounds
    once, and `x / 255 - mean` cancels near the mean: the largest distance is 27.4 ulp of the fp32 result (2.53e-7
    absolute; 453 of the 768 values differ from the rounded float64 result).  Without the normalisation the one fp32
    division IS the rounded quotient: 0 ulp.  A fact about the reference's arithmetic, which the device reproduces
    operation by operation — not a tolerance of any device test.  The assertion is the forward error bound of the three
    operations: the two roundings before the last division (half an ulp of a number below 1 each: 2^-25 + 2^-25) divided by
    the smallest std, plus half an ulp of a result below 4 (2^-23)."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    got = pc.to_float(u8)
    assert got.shape == (3, 16, 16) and got.dtype == torch.float32
    mean = np.asarray(pc.IMAGENET_MEAN, np.float32).astype(np.float64).reshape(3, 1, 1)
    std = np.asarray(pc.IMAGENET_STD, np.float32).astype(np.float64).reshape(3, 1, 1)
    x = np.moveaxis(u8, -1, 0).astype(np.float64)
    want = (x / 255.0 - mean) / std
    want32 = torch.from_numpy(want.astype(np.float32))
    ulp = torch.from_numpy(np.spacing(np.abs(want.astype(np.float32))).astype(np.float64))
    err = (got.double() - torch.from_numpy(want)).abs()
    print("to_float vs float64: largest distance %.3f ulp of the result, %.3e absolute; %d of 768 values differ from the "
          "rounded float64 result" % ((err / ulp).max().item(), err.max().item(), int((got != want32).sum())))
    assert err.max().item() <= 2.0 ** -24 / min(pc.IMAGENET_STD) * (1 + 2.0 ** -20) + 2.0 ** -23
    plain = pc.to_float(u8, mean=None)
    assert torch.equal(plain, torch.from_numpy((x / 255.0).astype(np.float32)))
    # the deterministic restatement is what the device tests share: it must not depend on the call
    assert torch.equal(got, pc.to_float(u8))


def test_pack_images_lays_dense_rows_back_to_back():
    imgs = [pc.case_image(c) for c in pc.CASES[2:5]]
    packed, desc = pc.pack_images(imgs)
    assert packed.dtype == np.uint8 and packed.shape == (sum(i.size for i in imgs),)
    for (off, h, w), im in zip(desc, imgs):
        assert np.array_equal(packed[off:off + 3 * h * w].reshape(h, w, 3), im)
