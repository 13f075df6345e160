"""Synthetic label cost volumes for TwoViewStereo's MRF stage: a noisy data term around a piecewise-smooth true labelling
(two planes and a step), an integer-valued variant (many exact ties), and masks.  Costs live where the pair costs live
(0 .. max_color_diff = 120); a fraction of the entries carries the fill value (2*5 + 1)*1000."""
import numpy as np

FILL = 11000.0


def truth(w, h, L):
    yy, xx = np.mgrid[0:h, 0:w]
    t = 0.2 * (L - 1) + 0.5 * (L - 1) * (xx / max(w - 1, 1)) * 0.6 + 0.1 * (L - 1) * np.sin(yy / 6.0)
    t = np.where((xx > w * 0.55) & (yy > h * 0.3), t * 0.4, t)             # a depth step
    return np.clip(np.rint(t), 0, L - 1).astype(np.int64)


def volume(w, h, L, seed=1, integer=False, mask_frac=0.85, fill_frac=0.03):
    """Returns (costs (h, w, L) float64, mask (h, w) uint8).  Masked-out pixels carry FILL on every label."""
    rng = np.random.default_rng(seed)
    tl = truth(w, h, L)
    lab = np.arange(L)[None, None, :]
    dist = np.abs(lab - tl[..., None]).astype(np.float64)
    costs = np.minimum(12.0 * dist, 90.0) + 30.0 * rng.uniform(size=(h, w, L))
    costs = np.minimum(costs, 120.0)
    if integer:
        costs = np.rint(costs / 8.0) * 2.0                                 # few distinct values, exact in every sum: ties
    costs = np.where(rng.uniform(size=(h, w, L)) < fill_frac, FILL, costs)
    mask = (rng.uniform(size=(h, w)) < mask_frac).astype(np.uint8)
    if mask_frac >= 1.0:
        mask[:] = 1
    costs = np.where(mask[..., None] == 1, costs, FILL)
    return np.ascontiguousarray(costs), mask
