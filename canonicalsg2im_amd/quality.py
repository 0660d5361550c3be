"""FID and the Inception score on the device: the two numbers results of this model are quoted by.

`FID(net)` accumulates the fp64 sum and outer product of the `dims`-wide Inception features of every picture it is given
(`ops.feat_stats`) and finalises them into the mean and the `np.cov` covariance on the device; `frechet_distance` is the
reference's `calculate_frechet_distance` (evaluation/fid/fid_score.py:136-190) on the host in numpy fp64, once per evaluation.
`InceptionScore(net)` keeps the fp32 softmax rows of every picture as float64 on the device and computes the reference's
`compute_score` (evaluation/inception.py:35-49) there.

LOADING THE REAL WEIGHT FILES AND THE NUMBERS THEY GIVE ARE UNCHECKED HERE (see inception.py): with `weights="random"` the
network is a seeded stand-in and `stand_in` is True on both classes — every output built on it says so.
"""
import numpy as np
import torch

from . import inception, ops


def _to_device_images(images, dev):
    if not torch.is_tensor(images):
        raise TypeError("images must be a tensor: uint8 (B,H,W,3) pictures or fp32 (B,3,H,W) images")
    if not images.is_cuda:
        raise RuntimeError("canonicalsg2im_amd.quality needs HIP (cuda) tensors; got a %s tensor — there is no CPU path"
                           % images.device)
    return images


class FID:
    """Feature statistics of one set of pictures.  `update(images)`: uint8 (B,H,W,3) pictures, or fp32 (B,3,H,W) images with
    values in [0, 1] — resized to 299 x 299, scaled to [-1, 1] and run through the network (inception.prepare, "fid").
    `statistics()` -> (mu (dims,), sigma (dims, dims)) as float64 host arrays."""

    def __init__(self, net, dims=2048, channel_order="rgb", size=(299, 299)):
        if net.variant != "fid":
            raise ValueError("FID needs InceptionV3('fid', ...), got the %r variant" % net.variant)
        if dims not in inception.DIMS:
            raise ValueError("FID: dims must be among %s" % (inception.DIMS,))
        self.net, self.dims, self.channel_order, self.size = net, dims, channel_order, size
        self.stand_in = net.stand_in
        self.clean()

    def clean(self):
        self.n, self._sum, self._outer = 0, None, None

    def features(self, images):
        """(B, dims) fp32 on the device."""
        images = _to_device_images(images, None)
        return self.net(inception.prepare(images, "fid", self.size, self.channel_order), dims=self.dims)

    def update(self, images):
        self.update_features(self.features(images))

    def update_features(self, feats):
        if self._sum is None:
            self._sum = torch.zeros(self.dims, device=feats.device, dtype=torch.float64)
            self._outer = torch.zeros(self.dims, self.dims, device=feats.device, dtype=torch.float64)
        ops.feat_stats(feats.contiguous(), self._sum, self._outer)
        self.n += int(feats.shape[0])

    def statistics(self):
        if self.n < 1:
            raise RuntimeError("FID.statistics: no picture was given")
        mu, sigma = ops.feat_stats_finalize(self._sum, self._outer, self.n)
        return mu.cpu().numpy(), sigma.cpu().numpy()


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """d^2 = |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr sqrtm(S1 S2), the reference's formula (fid_score.py:169-190), with
    tr sqrtm(S1 S2) = sum_i sqrt(max(Re lambda_i(S1 S2), 0)): the eigenvalues of a product of two positive semi-definite
    matrices are real and non-negative, so the trace of its principal square root is the sum of their roots — no scipy, and
    no `eps` fallback (the reference adds 1e-6 to the diagonals when `sqrtm` returns a non-finite matrix)."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise ValueError("Training and test covariances have different dimensions")
    if not (np.isfinite(sigma1).all() and np.isfinite(sigma2).all()):
        raise ValueError("frechet_distance: a covariance is not finite (statistics of a single picture?)")
    diff = mu1 - mu2
    lam = np.linalg.eigvals(sigma1.dot(sigma2))
    tr_covmean = np.sqrt(np.maximum(lam.real, 0.0)).sum()
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean)


def save_statistics(path, mu, sigma):
    """The `.npz` with `mu` and `sigma` the reference reads (fid_score.py:218-222)."""
    np.savez(path, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64))


def load_statistics(path):
    with np.load(path) as f:
        return f["mu"][:], f["sigma"][:]


class InceptionScore:
    """The reference's `InceptionScore(resize=True)` (evaluation/inception.py; scripts/train.py:341): `update(images)` resizes
    fp32 (B,3,H,W) images — the generator's output as it is, no rescaling — to 299 x 299, runs the network and keeps the
    softmax rows; `compute(splits)` -> (mean, std) of exp(mean KL(p(y|x) || p(y))) over the splits, Python floats;
    `clean()` forgets the rows.  uint8 pictures are accepted too (divided by 255)."""

    def __init__(self, net, channel_order="rgb", size=(299, 299)):
        if net.variant != "torchvision":
            raise ValueError("InceptionScore needs InceptionV3('torchvision', ...), got the %r variant" % net.variant)
        self.net, self.channel_order, self.size = net, channel_order, size
        self.stand_in = net.stand_in
        self.clean()

    def clean(self):
        self._rows = []

    def update(self, images):
        images = _to_device_images(images, None)
        logits = self.net(inception.prepare(images, "torchvision", self.size, self.channel_order))
        self._rows.append(ops.softmax_rows(logits))

    @property
    def n(self):
        return sum(int(r.shape[0]) for r in self._rows)

    def probabilities(self):
        """(N, 1000) float64 on the device."""
        if not self._rows:
            raise RuntimeError("InceptionScore: no picture was given")
        if len(self._rows) > 1:
            self._rows = [torch.cat(self._rows)]
        return self._rows[0]

    def compute(self, splits=1):
        out = ops.inception_score(self.probabilities(), splits).cpu()
        return float(out[0]), float(out[1])
