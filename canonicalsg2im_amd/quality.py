"""FID and the Inception score on the device: the two numbers results of this model are quoted by.

`FID(net)` accumulates the fp64 sum and outer product of the `dims`-wide Inception features of every picture it is given
(`ops.feat_stats`) and finalises them into the mean and the `np.cov` covariance on the device; `frechet_distance` is the
reference's `calculate_frechet_distance` (evaluation/fid/fid_score.py:136-190) on the host in numpy fp64, once per evaluation.
`InceptionScore(net)` keeps the fp32 softmax rows of every picture as float64 on the device and computes the reference's
`compute_score` (evaluation/inception.py:35-49) there.

Opt-in companions (csrc/quality.hip): `KID(net)` keeps the fp32 features and gives the unbiased kernel distance
over seeded subsets (`ops.kid_sums`, fp64, one fixed summation order); `ObjectFID(net)` is FID over the crops of every object's
box (SceneFID; `ops.crop_windows`, `ops.crop_resize_bilinear`) with per-class feature means (`ops.feat_class_sums`,
`class_mean_distance`: the reference's evaluation/fid.py:77-93); `crops_from_layouts` reads the boxes of a layouts.json.
`PRDC(net)` keeps the same features and gives improved precision / recall and density / coverage over k-nearest-neighbour
balls (csrc/manifold.hip: `ops.knn_radii`, `ops.ball_counts`, fp64 distances, integer counts, a stated tie rule).
Equality of these numbers with any other KID, SceneFID or precision / recall implementation is unchecked: the rules are this
project's own.

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


# ------------------------------------------------------------------------------------------------ KID
def kid_from_features(fx, fy, subsets=100, subset_size=1000, seed=0, degree=3, gamma=None, coef0=1.0):
    """KID (Binkowski et al. 2018) of two sets of feature rows, fp32 (n0,D) and (n1,D) on the device: the mean and the
    population std (np.std, ddof 0) over `subsets` subsets of the unbiased MMD^2 with k(u,v) = (gamma u.v + coef0)^degree,
    gamma = 1 / D unless given.  m = min(subset_size, n0, n1) rows per subset (a cap is printed and reported as
    `subset_size`); rng = np.random.RandomState(seed), per subset rng.choice(n0, m, replace=False) and then
    rng.choice(n1, m, replace=False).  One `ops.kid_sums` call, one read of its (S,3) sums; per subset
    MMD^2 = s0 / (m (m - 1)) + s1 / (m (m - 1)) - 2 s2 / m^2 in numpy fp64."""
    n0, n1 = int(fx.shape[0]), int(fy.shape[0])
    if n0 < 2 or n1 < 2:
        raise ValueError("KID needs at least 2 rows per side, got %d and %d" % (n0, n1))
    subsets, subset_size = int(subsets), int(subset_size)
    if subsets < 1 or subset_size < 2:
        raise ValueError("KID: subsets must be >= 1 and subset_size >= 2, got %d and %d" % (subsets, subset_size))
    m = min(subset_size, n0, n1)
    if m < subset_size:
        print("KID: subset_size %d capped to %d, the smaller side" % (subset_size, m))
    gamma = 1.0 / int(fx.shape[1]) if gamma is None else float(gamma)
    rng = np.random.RandomState(seed)
    ix, iy = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(n0, m, replace=False)
        iy[s] = rng.choice(n1, m, replace=False)
    sums = ops.kid_sums(fx.contiguous(), fy.contiguous(), torch.from_numpy(ix).to(fx.device), torch.from_numpy(iy).to(fx.device),
                        gamma, coef0, degree).cpu().numpy()
    mmd2 = sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)
    return {"mean": float(np.mean(mmd2)), "std": float(np.std(mmd2)), "subsets": subsets, "subset_size": m, "n": [n0, n1]}


class KID:
    """KID of two sets of pictures over the features FID uses: `update(images, which)` (which 0 or 1; uint8 (B,H,W,3)
    pictures or fp32 (B,3,H,W) images, prepared as for FID) or `update_features(feats, which)` keep the fp32 features on
    the device; `compute()` -> {"mean", "std", "subsets", "subset_size", "n": [n0, n1], "stand_in"} (kid_from_features)."""

    def __init__(self, net, dims=2048, channel_order="rgb", size=(299, 299), subsets=100, subset_size=1000, seed=0, degree=3,
                 gamma=None, coef0=1.0):
        if net.variant != "fid":
            raise ValueError("KID needs InceptionV3('fid', ...), got the %r variant" % net.variant)
        if dims not in inception.DIMS:
            raise ValueError("KID: dims must be among %s" % (inception.DIMS,))
        self.net, self.dims, self.channel_order, self.size = net, dims, channel_order, size
        self.subsets, self.subset_size, self.seed = subsets, subset_size, seed
        self.degree, self.gamma, self.coef0 = degree, gamma, coef0
        self.stand_in = net.stand_in
        self.clean()

    def clean(self):
        self._feats = ([], [])

    @staticmethod
    def _which(which):
        if which not in (0, 1):
            raise ValueError("KID: which must be 0 or 1, got %r" % (which,))
        return which

    def update(self, images, which):
        self._which(which)
        images = _to_device_images(images, None)
        self.update_features(self.net(inception.prepare(images, "fid", self.size, self.channel_order), dims=self.dims), which)

    def update_features(self, feats, which):
        if feats.dim() != 2 or feats.shape[1] != self.dims or feats.dtype != torch.float32:
            raise ValueError("KID: features must be fp32 (n, %d), got %s %s" % (self.dims, feats.dtype, tuple(feats.shape)))
        self._feats[self._which(which)].append(feats.detach())

    @property
    def n(self):
        return [sum(int(f.shape[0]) for f in side) for side in self._feats]

    def compute(self):
        n0, n1 = self.n
        if n0 < 2 or n1 < 2:
            raise ValueError("KID needs at least 2 pictures per side, got %d and %d" % (n0, n1))
        fx, fy = (torch.cat(side) for side in self._feats)
        out = kid_from_features(fx, fy, self.subsets, self.subset_size, self.seed, self.degree,
                                1.0 / self.dims if self.gamma is None else self.gamma, self.coef0)
        out["stand_in"] = bool(self.stand_in)
        return out


# ------------------------------------------------------------------------------------------------ precision / recall, density / coverage
def prdc_from_features(real, gen, k=5):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of two sets of
    feature rows, fp32 (n_real,D) and (n_gen,D) on the device, over k-nearest-neighbour balls: the radius of
    a row is the distance to its k-th nearest OTHER row of its own set (`ops.knn_radii`), and with
    inside = ops.ball_counts(gen, real, r_real)[0], holds = ...[1] and inside_r = ops.ball_counts(real, gen, r_gen)[0]

        precision = mean(inside > 0)      density  = sum(inside) / (k n_gen)
        recall    = mean(inside_r > 0)    coverage = mean(holds > 0)

    The four integer sums are formed on the device and read once; the divisions happen on the host.  k = 5 is the default
    of the `prdc` package, which reports all four with one k; the improved precision and recall paper uses k = 3.
    Non-finite features and k >= min(n_real, n_gen) are refused.
    -> {"precision", "recall", "density", "coverage", "k", "n": [n_real, n_gen]}"""
    for t, name in ((real, "real"), (gen, "generated")):
        if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError("PRDC: the %s features must be an fp32 (n,D) tensor" % name)
    if real.shape[1] != gen.shape[1]:
        raise ValueError("PRDC: the two sides differ in width: %d and %d" % (real.shape[1], gen.shape[1]))
    n_real, n_gen, k = int(real.shape[0]), int(gen.shape[0]), int(k)
    if k < 1 or k >= min(n_real, n_gen):
        raise ValueError("PRDC: k = %d needs 1 <= k < min(n_real, n_gen) = %d rows: a row's radius is the distance to its "
                         "k-th nearest other row" % (k, min(n_real, n_gen)))
    real, gen = real.detach().contiguous(), gen.detach().contiguous()
    _to_device_images(real, None), _to_device_images(gen, None)
    # a side's largest and smallest entry (torch's max and min hand a NaN on): no temporary the size of the features
    ends = torch.isfinite(torch.stack([real.amax(), real.amin(), gen.amax(), gen.amin()])).cpu().tolist()
    for ok, name in zip((ends[0] and ends[1], ends[2] and ends[3]), ("real", "generated")):
        if not ok:
            raise ValueError("PRDC: the %s features hold a NaN or an infinity: a ball around such a row means nothing" % name)
    inside, holds = ops.ball_counts(gen, real, ops.knn_radii(real, k))
    inside_r, _ = ops.ball_counts(real, gen, ops.knn_radii(gen, k))
    sums = torch.stack([(inside > 0).sum(), (inside_r > 0).sum(), inside.sum(dtype=torch.int64), (holds > 0).sum()]).cpu().tolist()
    return {"precision": sums[0] / n_gen, "recall": sums[1] / n_real, "density": sums[2] / (k * n_gen),
            "coverage": sums[3] / n_real, "k": k, "n": [n_real, n_gen]}


class PRDC:
    """Precision, recall, density and coverage of two sets of pictures over the features FID uses: `update(images, which)`
    (which 0 = real, 1 = generated; uint8 (B,H,W,3) pictures or fp32 (B,3,H,W) images, prepared as for FID) or
    `update_features(feats, which)` keep the fp32 features on the device; `compute()` -> prdc_from_features's dict with
    "stand_in"."""

    def __init__(self, net, dims=2048, channel_order="rgb", size=(299, 299), k=5):
        if net.variant != "fid":
            raise ValueError("PRDC needs InceptionV3('fid', ...), got the %r variant" % net.variant)
        if dims not in inception.DIMS:
            raise ValueError("PRDC: dims must be among %s" % (inception.DIMS,))
        if int(k) < 1:
            raise ValueError("PRDC: k must be at least 1, got %r" % (k,))
        self.net, self.dims, self.channel_order, self.size, self.k = net, dims, channel_order, size, int(k)
        self.stand_in = net.stand_in
        self.clean()

    def clean(self):
        self._feats = ([], [])

    @staticmethod
    def _which(which):
        if which not in (0, 1):
            raise ValueError("PRDC: which must be 0 (real) or 1 (generated), got %r" % (which,))
        return which

    def update(self, images, which):
        self._which(which)
        images = _to_device_images(images, None)
        self.update_features(self.net(inception.prepare(images, "fid", self.size, self.channel_order), dims=self.dims), which)

    def update_features(self, feats, which):
        if feats.dim() != 2 or feats.shape[1] != self.dims or feats.dtype != torch.float32:
            raise ValueError("PRDC: features must be fp32 (n, %d), got %s %s" % (self.dims, feats.dtype, tuple(feats.shape)))
        self._feats[self._which(which)].append(feats.detach())

    @property
    def n(self):
        return [sum(int(f.shape[0]) for f in side) for side in self._feats]

    def compute(self):
        n0, n1 = self.n
        if self.k >= min(n0, n1):
            raise ValueError("PRDC: k = %d needs more than k pictures per side, got %d and %d" % (self.k, n0, n1))
        real, gen = (torch.cat(side) for side in self._feats)
        out = prdc_from_features(real, gen, self.k)
        out["stand_in"] = bool(self.stand_in)
        return out


# ------------------------------------------------------------------------------------------------ object-level FID
def _host_rows(what, values, dtype, width):
    a = np.asarray(values, dtype=dtype)
    if a.ndim != (2 if width else 1) or (width and a.shape[1] != width):
        raise ValueError("ObjectFID: %s must be %s, got an array of shape %s" % (
            what, "(N,%d)" % width if width else "(N,)", a.shape))
    return a


class ObjectFID(FID):
    """SceneFID (Sylvain et al. 2021): FID over the crops of every object's box.  `update(pictures_u8, boxes, image_index,
    class_ids=None)`: uint8 (B,H,W,3) pictures on the device, boxes (N,4) [x, y, w, h] in units of the picture, image_index
    (N) — host arrays (checked: finite values, index in range, ValueError naming the row) or device tensors.  `batch_size`
    crops at a time, the remainder batch included: ops.crop_windows, ops.crop_resize_bilinear with the "fid" affine (2, -1),
    the network, ops.feat_stats and, with class_ids (integers into `classes`), ops.feat_class_sums.  `statistics()` as
    FID's; `class_means()` -> (means (C,dims) float64, NaN for a class without crops; counts (C) int64)."""

    def __init__(self, net, dims=2048, channel_order="rgb", size=(299, 299), batch_size=50, classes=None):
        super().__init__(net, dims=dims, channel_order=channel_order, size=size)
        if int(batch_size) < 1:
            raise ValueError("ObjectFID: batch_size must be positive")
        self.batch_size = int(batch_size)
        self.classes = None if classes is None else list(classes)

    def clean(self):
        super().clean()
        self._class_sums, self._class_counts = None, None

    def _operands(self, pictures, boxes, image_index, class_ids):
        pictures = _to_device_images(pictures, None)
        if pictures.dtype != torch.uint8 or pictures.dim() != 4 or pictures.shape[3] != 3:
            raise ValueError("ObjectFID: pictures must be uint8 (B,H,W,3), got %s %s" % (pictures.dtype, tuple(pictures.shape)))
        dev, B = pictures.device, int(pictures.shape[0])
        if not torch.is_tensor(boxes):
            host = _host_rows("boxes", boxes, np.float32, 4)
            bad = np.flatnonzero(~np.isfinite(host).all(axis=1))
            if bad.size:
                raise ValueError("ObjectFID: boxes row %d is not finite: %s" % (int(bad[0]), host[bad[0]].tolist()))
            boxes = torch.from_numpy(np.ascontiguousarray(host))
        if not torch.is_tensor(image_index):
            host = _host_rows("image_index", image_index, np.int64, 0)
            bad = np.flatnonzero((host < 0) | (host >= B))
            if bad.size:
                raise ValueError("ObjectFID: image_index row %d is %d, outside the %d pictures" % (
                    int(bad[0]), int(host[bad[0]]), B))
            image_index = torch.from_numpy(host)
        boxes = boxes.to(device=dev, dtype=torch.float32).contiguous()
        image_index = image_index.to(device=dev, dtype=torch.int32).contiguous()
        N = int(boxes.shape[0])
        if boxes.dim() != 2 or boxes.shape[1] != 4 or N < 1 or tuple(image_index.shape) != (N,):
            raise ValueError("ObjectFID: boxes must be (N,4) and image_index (N,) with N >= 1, got %s and %s" % (
                tuple(boxes.shape), tuple(image_index.shape)))
        if class_ids is not None:
            if self.classes is None:
                raise ValueError("ObjectFID: class_ids need ObjectFID(classes=[...]): the ids index that list")
            if not torch.is_tensor(class_ids):
                class_ids = torch.from_numpy(_host_rows("class_ids", class_ids, np.int64, 0))
            class_ids = class_ids.to(device=dev, dtype=torch.int32).contiguous()
            if tuple(class_ids.shape) != (N,):
                raise ValueError("ObjectFID: class_ids must be (N,) = (%d,), got %s" % (N, tuple(class_ids.shape)))
        return pictures.contiguous(), boxes, image_index, class_ids

    def _batches(self, pictures, boxes, image_index):
        """(first crop, features) of every batch of `batch_size` crops, the remainder batch included."""
        reverse = self.channel_order == "bgr"
        windows = ops.crop_windows(boxes, pictures.shape[1], pictures.shape[2])
        for i in range(0, int(boxes.shape[0]), self.batch_size):
            j = i + self.batch_size
            x = ops.crop_resize_bilinear(pictures, windows[i:j], image_index[i:j], self.size, 2.0, -1.0, reverse=reverse)
            yield i, self.net(x, dims=self.dims)

    def features(self, pictures, boxes, image_index):
        """(N, dims) fp32 on the device: the features of the crops, in row order."""
        pictures, boxes, image_index, _ = self._operands(pictures, boxes, image_index, None)
        return torch.cat([f for _, f in self._batches(pictures, boxes, image_index)])

    def update(self, pictures, boxes, image_index, class_ids=None):
        """-> the (N, dims) features it accumulated (for `KID` on crops)."""
        pictures, boxes, image_index, class_ids = self._operands(pictures, boxes, image_index, class_ids)
        kept = []
        for i, feats in self._batches(pictures, boxes, image_index):
            self.update_features(feats, None if class_ids is None else class_ids[i:i + self.batch_size])
            kept.append(feats)
        return torch.cat(kept)

    def update_features(self, feats, class_ids=None):
        super().update_features(feats)
        if class_ids is None:
            return
        if self._class_sums is None:
            C = len(self.classes)
            self._class_sums = torch.zeros(C, self.dims, device=feats.device, dtype=torch.float64)
            self._class_counts = torch.zeros(C, device=feats.device, dtype=torch.int64)
        ops.feat_class_sums(feats.contiguous(), class_ids.contiguous(), self._class_sums, self._class_counts)

    def class_means(self):
        if self._class_sums is None:
            raise RuntimeError("ObjectFID.class_means: no crop with a class was given")
        sums, counts = self._class_sums.cpu().numpy(), self._class_counts.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            return sums / counts[:, None].astype(np.float64), counts


def class_mean_distance(means_a, counts_a, means_b, counts_b, min_crops=1):
    """Per class with at least `min_crops` crops on both sides, |mu_b - mu_a|^2 of the class's feature means, and the mean of
    those distances: the reference's per-class `get_fid` (evaluation/fid.py:77-93).  A class that has `min_crops` crops on
    one side only is listed under "missing" and not averaged.  -> {"mean", "per_class": {class index: distance}, "missing"}."""
    means_a, means_b = np.asarray(means_a, np.float64), np.asarray(means_b, np.float64)
    counts_a, counts_b = np.asarray(counts_a), np.asarray(counts_b)
    if means_a.shape != means_b.shape or counts_a.shape != counts_b.shape or counts_a.shape != means_a.shape[:1]:
        raise ValueError("class_mean_distance: the two sides must have the same (C,dims) means and (C,) counts")
    need = max(int(min_crops), 1)
    per_class, missing = {}, []
    for c in range(means_a.shape[0]):
        in_a, in_b = counts_a[c] >= need, counts_b[c] >= need
        if in_a and in_b:
            diff = means_b[c] - means_a[c]
            per_class[c] = float(diff.dot(diff))
        elif in_a or in_b:
            missing.append(c)
    mean = float(np.mean(list(per_class.values()))) if per_class else float("nan")
    return {"mean": mean, "per_class": per_class, "missing": missing}


def crops_from_layouts(doc, which="gt", min_object_size=0.0):
    """Host only.  `doc`: the dict of a layouts.json (scripts.sample --split).  -> {image id: (boxes [n][4], class keys [n])}
    of the rows kept: `gt_boxes`, or `predicted_boxes` with which="pred".  The class key is the row's `objects` entry, or
    json.dumps(entry, sort_keys=True) when it is not a string.  A row whose w * h < min_object_size, or whose box is not
    finite, is left out."""
    import json
    if which not in ("gt", "pred"):
        raise ValueError("crops_from_layouts: which must be 'gt' or 'pred', got %r" % (which,))
    if not isinstance(doc, dict) or not isinstance(doc.get("images"), list):
        raise ValueError("crops_from_layouts: the document has no 'images' list")
    key = "gt_boxes" if which == "gt" else "predicted_boxes"
    out = {}
    for index, row in enumerate(doc["images"]):
        for need in ("image_id", "objects", key):
            if need not in row:
                raise ValueError("crops_from_layouts: images[%d] has no %r%s" % (
                    index, need, " (which='pred' needs the rows of a run that predicted boxes)" if need == "predicted_boxes" else ""))
        names, boxes = row["objects"], row[key]
        if len(names) != len(boxes):
            raise ValueError("crops_from_layouts: images[%d] has %d objects and %d %s" % (index, len(names), len(boxes), key))
        kept_boxes, kept_keys = [], []
        for name, box in zip(names, boxes):
            box = [float(v) for v in box]
            if len(box) != 4 or not all(np.isfinite(box)) or box[2] * box[3] < min_object_size:
                continue
            kept_boxes.append(box)
            kept_keys.append(name if isinstance(name, str) else json.dumps(name, sort_keys=True))
        if row["image_id"] in out:
            raise ValueError("crops_from_layouts: image id %r a second time" % (row["image_id"],))
        out[row["image_id"]] = (kept_boxes, kept_keys)
    return out
