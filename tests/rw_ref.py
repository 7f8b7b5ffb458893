"""float64 restatement of the random-walker contract (include/wsl_hip.h, "random-walker pseudo labels"): the graph Laplacian of the
4-connected grid assembled with scipy.sparse and solved directly with splu.  Test helper only -- nothing in the package imports it.

    d = 2 (clip(I, -0.35, 1.35) + 0.35) / 1.7 - 1,   w_pq = exp(-beta (d_p - d_q)^2 / (10 std(d))) + 1e-6   (std == 0: w = 1 + 1e-6)
    L = D - W,   L_uu x_k = -L_um [S_m == k],   label = argmax_k x_k (ties to the lowest class), seeds kept
    a slice whose seeds lack one of the classes 1 .. K-1 is all zeros

Also the synthetic inputs of tests/test_random_walker.py and a cache, so a reference is computed once per input and shared."""
import os

import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUME = os.path.join(ROOT, "tests", "golden", "acdc", "ACDC_training_volumes", "patient041_frame11.h5")
SLICES = os.path.join(ROOT, "tests", "golden", "acdc", "ACDC_training_slices")


def class_rule(seed, K):
    return all(k in seed for k in range(1, K))


def system(img, seed, K, beta=100.0):
    """-> (L_uu csc, B [nu, K] dense, u: flat indices of the unlabelled pixels) in float64"""
    H, W = img.shape
    d = 2.0 * (np.clip(img.astype(np.float64), -0.35, 1.35) + 0.35) / 1.7 - 1.0
    std = d.std()
    constant = std == 0 or np.all(d == d.flat[0])        # (numpy's mean of n equal doubles can be an ulp off: std 1e-17, not 0)

    def wt(a, b):
        return (np.ones_like(a) if constant else np.exp(-beta * (a - b) ** 2 / (10.0 * std))) + 1e-6

    idx = np.arange(H * W).reshape(H, W)
    i = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    j = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    w = np.concatenate([wt(d[:, :-1], d[:, 1:]).ravel(), wt(d[:-1, :], d[1:, :]).ravel()])
    Wm = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(H * W, H * W)).tocsr()
    L = sparse.diags(np.asarray(Wm.sum(1)).ravel()) - Wm
    s = seed.ravel().astype(np.int64)
    u, m = np.nonzero(s >= K)[0], np.nonzero(s < K)[0]
    onehot = (s[m][:, None] == np.arange(K)[None, :]).astype(np.float64)
    L = L.tocsr()
    return L[u][:, u].tocsc(), -(L[u][:, m] @ onehot), u


def solve(img, seed, K, beta=100.0):
    """one slice -> dict(prob [K, H, W] f64 (one-hot on seeds), label [H, W] u8, gap [H, W]: the top-two margin, Luu, B, u)"""
    H, W = img.shape
    s = seed.astype(np.int64)
    if not class_rule(seed, K):
        return dict(prob=np.zeros((K, H, W)), label=np.zeros((H, W), np.uint8), gap=np.ones((H, W)), Luu=None, B=None, u=None)
    Luu, B, u = system(img, seed, K, beta)
    prob = (s.ravel()[None, :] == np.arange(K)[:, None]).astype(np.float64)
    if u.size:
        prob[:, u] = splu(Luu).solve(B).T
    prob = prob.reshape(K, H, W)
    label = np.argmax(prob, 0).astype(np.uint8)             # (first maximum: the lowest class)
    top = np.sort(prob, 0)
    gap = top[-1] - top[-2]
    gap[s < K] = 1.0
    return dict(prob=prob, label=label, gap=gap, Luu=Luu, B=B, u=u)


def true_residuals(ref, prob):
    """|b_k - L_uu x_k| / |b_k| per class in float64 for returned probabilities [K, H, W] (0 where b_k = 0)"""
    x = prob.reshape(prob.shape[0], -1)[:, ref["u"]].astype(np.float64).T
    r = ref["B"] - ref["Luu"] @ x
    bn = np.linalg.norm(ref["B"], axis=0)
    return np.where(bn > 0, np.linalg.norm(r, axis=0) / np.where(bn > 0, bn, 1.0), 0.0)


_cache = {}


def cached(key, img, seed, K, beta=100.0):
    """solve() of every slice of a batch, computed once per key; callers must not modify the result"""
    if key not in _cache:
        _cache[key] = [solve(i, s, K, beta) for i, s in zip(img, seed)]
    return _cache[key]


# ---------------------------------------------------------------------------------------------- inputs
def _synthetic_one(H, W, noise):
    cy, cx, m = H // 2, W // 2, min(H, W)
    yy, xx = np.mgrid[:H, :W]
    r2 = (yy - cy) ** 2 + (xx - cx) ** 2
    img = np.clip(0.2 + 0.5 * (r2 < (m / 3) ** 2) + 0.2 * (r2 < (m / 6) ** 2) + 0.03 * noise, 0, 1).astype(np.float32)
    seed = np.full((H, W), 4, np.uint8)
    seed[1, 1:W - 1] = 0
    seed[cy, cx - 1:cx + 2] = 1
    q = m // 4
    seed[cy - q - 2:cy - q + 2, cx] = 2                    # 4 pixels around the row a quarter of the short side above the centre
    seed[cy + q - 2:cy + q + 2, cx] = 3                    # ... and below it
    return img, seed


def synthetic():
    """{(24, 20): (img [2, H, W] f32, seed [2, H, W] u8), (33, 47): ...}: a bright disc with a brighter core on a dark background plus
    noise from default_rng(0) (drawn for 24 x 20 first, then 33 x 47); class 0 on row 1, class 1 on 3 pixels at the centre, classes 2 and
    3 on 4 pixels of the centre column a quarter of the short side above and below it.  The second slice is the first one flipped in
    both axes."""
    if "synthetic" not in _cache:
        rng = np.random.default_rng(0)
        out = {}
        for H, W in ((24, 20), (33, 47)):
            img, seed = _synthetic_one(H, W, rng.standard_normal((H, W)))
            out[(H, W)] = (np.stack([img, img[::-1, ::-1]]).copy(), np.stack([seed, seed[::-1, ::-1]]).copy())
        _cache["synthetic"] = out
    return _cache["synthetic"]


def volume():
    """(image [D, 224, 154] f32, scribble [D, 224, 154] u8) of the committed ACDC volume"""
    if "volume" not in _cache:
        from wsl4mis_amd.dataloaders import h5lite
        with h5lite.File(VOLUME) as f:
            _cache["volume"] = (f["image"][:].astype(np.float32), f["scribble"][:].astype(np.uint8))
    return _cache["volume"]
