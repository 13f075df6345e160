"""The constants of srh_params / sro_params as an axis of the parity suite: one table of (case, override) entries shared by
tests/test_constants_host.py (the oracle alone: every override changes what its witness says it changes, so no device
case is vacuous) and tests/test_gpu_constants.py (every kernel path against the oracle under the override).

An entry names a case of tests/cases.py at a small shape (shapes are the subject of other suites), the overridden
parameters, a WITNESS -- what the override has to move on the oracle -- and the share of pixels it moves, measured on the
oracle and written down as a literal (`share`); the host test asserts the measured share is at least `MIN_SHARE` and
within 1.5 points of that literal.

  witness "depth"   the left -> right WTA map (MVS: view 0's initial estimate) differs in bits from the default-constants map
  witness "peaks"   MVS: view 0's top-K peak lists differ from the default ones (shorter lists padded at the front with
                    the empty entry (0, -1), which is where the oracle keeps them)
  witness "cross"   the cross-checked pair of maps (sro_twoview_cross_check on the oracle's two WTA maps) changes class
  witness "branch"  no share: the override is known from the code to switch a kernel branch (`sdiv`, below)

Only numpy and the oracle here; oracle results are cached per entry and handed out read-only."""
import collections
import functools
import math

import numpy as np

import cases

MIN_SHARE = 0.02

# case -> shape
SHAPES = {
    "geodesic_rect": dict(w=96, h=40, D=24), "geodesic_masks": dict(w=96, h=40, D=24),
    "adaptive_rect": dict(w=96, h=40, D=24), "adaptive_masks": dict(w=96, h=40, D=24),
    "geodesic_r2": dict(w=96, h=40, D=24),
    "geodesic_verged_dist_masks": dict(w=64, h=40, D=16),
    "mvs_geodesic": dict(w=48, h=36, D=20, nviews=3),
}
RECTIFIED = ("geodesic_rect", "geodesic_masks", "adaptive_rect", "adaptive_masks", "geodesic_r2")

Entry = collections.namedtuple("Entry", "case over witness share")


def _e(case, witness, share, **over):
    return Entry(case, tuple(sorted(over.items())), witness, share)


# `share`: measured on the oracle (tests/test_constants_host.py prints and re-asserts every one)
ENTRIES = [
    _e("geodesic_rect", "depth", 0.717, geodesic_sigma=7.3),
    _e("geodesic_rect", "depth", 0.501, geodesic_sigma=400.0),
    _e("geodesic_rect", "depth", 0.816, geodesic_sigma=0.5),
    _e("geodesic_rect", "depth", 0.642, geodesic_sigma=1e6),
    _e("geodesic_rect", "depth", 0.123, geodesic_iters=1),
    _e("geodesic_rect", "depth", 0.808, geodesic_iters=0),
    _e("geodesic_rect", "depth", 0.482, geodesic_init=30.0),
    _e("geodesic_rect", "depth", 0.642, geodesic_init=0.0),
    _e("geodesic_rect", "depth", 0.551, geodesic_init=-100.0),
    _e("geodesic_rect", "depth", 0.707, geodesic_sigma=-50.0),
    _e("geodesic_rect", "depth", 0.334, weight_cutoff=0.3),
    _e("geodesic_rect", "depth", 0.736, weight_cutoff=0.7),
    # (bad_ret moves no depth on these pairs -- a candidate's centre tap is always usable, and where nothing else is, the
    # lone bad_ret still "wins" -- but it IS the winner's cost of 0.9 % of the pixels here: the planes of wta_outputs see it.
    # Random pairs meet it far more often: pairs(), below.)
    _e("geodesic_rect", "depth", 0.742, weight_cutoff=0.7, bad_ret=0.02),
    _e("geodesic_rect", "depth", 0.576, second_best_factor=0.6),
    _e("geodesic_rect", "depth", 0.180, second_best_factor=1.5),
    _e("geodesic_rect", "depth", 0.808, wta_margin=2.0),
    _e("geodesic_masks", "depth", 0.109, max_color_diff=0.3),
    _e("geodesic_masks", "depth", 0.494, max_color_diff=0.05),
    _e("geodesic_masks", "depth", 0.451, weight_cutoff=0.7),
    _e("geodesic_masks", "depth", 0.180, weight_cutoff=0.3, bad_ret=0.02),
    _e("adaptive_rect", "depth", 0.607, adaptive_color_sigma=2.5),
    _e("adaptive_rect", "depth", 0.563, adaptive_color_sigma=60.0),
    _e("adaptive_rect", "depth", 0.284, weight_cutoff=0.05),
    _e("adaptive_masks", "depth", 0.436, weight_cutoff=0.3, bad_ret=0.02),
    _e("geodesic_r2", "depth", 0.673, weight_cutoff=0.7),
    _e("geodesic_r2", "depth", 0.343, geodesic_init=-100.0),
    _e("geodesic_r2", "depth", 0.830, geodesic_sigma=0.5),
    _e("geodesic_verged_dist_masks", "depth", 0.327, geodesic_sigma=7.3),
    _e("geodesic_verged_dist_masks", "depth", 0.029, geodesic_iters=1),
    _e("geodesic_verged_dist_masks", "depth", 0.403, geodesic_iters=0),
    _e("geodesic_verged_dist_masks", "depth", 0.080, geodesic_init=30.0),
    _e("mvs_geodesic", "depth", 0.262, geodesic_sigma=7.3),
    _e("mvs_geodesic", "depth", 0.022, geodesic_iters=1),
    _e("mvs_geodesic", "depth", 0.060, weight_cutoff=0.3),
    _e("mvs_geodesic", "depth", 0.190, num_neighbours=1),
    _e("mvs_geodesic", "depth", 0.190, neighbour_min_dot=0.95),
    # no depth has to move: the witness is the peak list.  Every score the oracle computes on this case lies in
    # [0.985, 0.99995] (the views of the sphere are smooth and close), so 0.8 moves NOTHING (share 0) and 0.99 moves 0.23 %
    # of the lists: the thresholds are the 5 % and the 50 % quantile of the oracle's default peak costs (0.99517, 0.99759).
    _e("mvs_geodesic", "peaks", 0.042, peak_threshold=0.995),
    _e("mvs_geodesic", "peaks", 0.245, peak_threshold=0.9976),     # (this one moves depths too)
    _e("mvs_geodesic", "peaks", 0.341, top_k=3),
    # crossCheck only: 0.25 and 4 (default 1) both change the class of more than 2 % of the pixels of the two maps
    _e("geodesic_rect", "cross", 0.143, inconsistency_thresh=0.25),
    _e("geodesic_rect", "cross", 0.120, inconsistency_thresh=4.0),
    # branches of the windows kernels (sdiv false); every weight but the centre's 0 and every cost NaN -> clamp at 5e-4
    _e("geodesic_rect", "branch", None, geodesic_init=1e300),
    _e("geodesic_rect", "branch", None, geodesic_sigma=5e-4),
]

# SAD (option "cost" = 1, tests/sad_ref.py): witness "sad", the left -> right SAD map against the default-constants SAD map.
# cost_sad clamps per tap, grey differences live in [0, 255] and winning costs around 2 .. 25: max_color_diff 40 moves
# nothing, 20 moves 8.9 %, 10 moves 19.7 % (chosen); bad_ret 2.0 lies inside the cost range, and at weight_cutoff 0.7 it is
# the winning cost of 23 % of the pixels of geodesic_masks (windows left with four taps or fewer).
SAD_ENTRIES = [
    _e("geodesic_rect", "sad", 0.654, geodesic_sigma=7.3),
    _e("geodesic_rect", "sad", 0.070, geodesic_iters=1),
    _e("geodesic_masks", "sad", 0.424, weight_cutoff=0.7, bad_ret=2.0),
    _e("geodesic_masks", "sad", 0.197, max_color_diff=10.0),
    _e("adaptive_rect", "sad", 0.418, adaptive_color_sigma=2.5),
    _e("adaptive_masks", "sad", 0.492, weight_cutoff=0.3, bad_ret=0.02),
]


def entry_id(e):
    return "%s-%s" % (e.case, "-".join("%s=%g" % kv for kv in e.over)) if e.over else e.case + "-defaults"


def entries(witness=None, case=None, kind=None, has=None):
    """the table filtered: by witness, by case name(s), by kind ("twoview" / "mvs"), by an overridden parameter"""
    out = []
    for e in ENTRIES:
        if witness is not None and e.witness not in (witness if isinstance(witness, tuple) else (witness,)):
            continue
        if case is not None and e.case not in (case if isinstance(case, tuple) else (case,)):
            continue
        if kind is not None and (e.case.startswith("mvs")) != (kind == "mvs"):
            continue
        if has is not None and not any(k in dict(e.over) for k in has):
            continue
        out.append(e)
    return out


def default_entry(case):
    return Entry(case, (), "depth", None)


def sdiv(params):
    """the predicate of geodesic_reg_kernel / geodesic_dma_kernel (csrc/srh_dense.hip) that selects the shared-divisor
    division and the range-select-free exp; `params` is the override dict on top of the defaults (50, 1e6)"""
    sigma = params.get("geodesic_sigma", 50.0)
    init = params.get("geodesic_init", 1e6)
    return sigma > 0 and 2.0 ** -300 < init < 2.0 ** 300 and init < 2.0 ** 30 * sigma


def median_premise(over):
    """the host check of srh_view_filter_invalid with SRH_FILTER_MEDIAN and geodesic windows (include/stereo_recon_hip.h)"""
    sigma, init = over.get("geodesic_sigma", 50.0), over.get("geodesic_init", 1e6)
    if not sigma > 0:
        return False
    try:
        return math.exp(-init / sigma) <= 1e-10
    except OverflowError:
        return False


@functools.lru_cache(maxsize=None)
def build(e):
    """-> the case dict of tests/cases.py with the entry's overrides in its params"""
    mk = cases.get_mvs if e.case.startswith("mvs") else cases.get_twoview
    case = mk(e.case, **SHAPES[e.case])
    case["params"] = dict(case["params"], **dict(e.over))
    return case


@functools.lru_cache(maxsize=None)
def oracle_inputs(e):
    return cases.oracle_inputs(build(e))


@functools.lru_cache(maxsize=None)
def oracle_twoview(e, direction):
    """(depth, diag) of one oracle pass: direction 0 is left -> right.  Read-only, computed once."""
    import oracle_ffi as O
    imgs, cams, p = oracle_inputs(e)
    r, o = (0, 1) if direction == 0 else (1, 0)
    depth, diag = O.twoview_wta(imgs[r], imgs[o], cams[r], cams[o], p, want_diag=True)
    depth.setflags(write=False)
    for k in ("win_xy", "min_cost", "second_cost"):
        diag[k].setflags(write=False)
    return depth, diag


@functools.lru_cache(maxsize=None)
def oracle_cross(e):
    """the oracle's chain: both WTA passes, then crossCheck"""
    import oracle_ffi as O
    imgs, cams, p = oracle_inputs(e)
    cl, cr = O.twoview_cross_check(cams[0], cams[1], p, oracle_twoview(e, 0)[0], oracle_twoview(e, 1)[0])
    cl.setflags(write=False)
    cr.setflags(write=False)
    return cl, cr


@functools.lru_cache(maxsize=None)
def oracle_neighbours(e):
    import oracle_ffi as O
    imgs, cams, p = oracle_inputs(e)
    return tuple(tuple(int(n) for n in v) for v in O.mvs_neighbours(cams, p))


@functools.lru_cache(maxsize=None)
def oracle_mvs(e, view):
    """(depth, peaks, n_eval) of one view's initial estimate"""
    import oracle_ffi as O
    imgs, cams, p = oracle_inputs(e)
    depth, peaks, n_eval = O.mvs_initial_estimate(imgs, cams, view, list(oracle_neighbours(e)[view]), p, want_peaks=True)
    depth.setflags(write=False)
    peaks.setflags(write=False)
    return depth, peaks, n_eval


def pairs(e, n=600):
    """n random (x1, y1, x2, y2) for srh_twoview_pair_costs: reference pixels anywhere, candidates up to 3 pixels outside"""
    case = build(e)
    h, w = case["views"][0][0].shape[:2]
    rng = np.random.default_rng(0xC0575 + len(entry_id(e)))
    return np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(-3, w + 3, n), rng.integers(-3, h + 3, n)], 1).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def oracle_sad(e, direction):
    """(depth, min cost) of one SAD pass of the CPU restatement (tests/sad_ref.py)"""
    import sad_ref as S
    imgs, cams, p = oracle_inputs(e)
    r, o = (0, 1) if direction == 0 else (1, 0)
    depth, mc = S.twoview_wta_sad(imgs[r], imgs[o], cams[r], cams[o], p, want_cost=True)
    depth.setflags(write=False)
    mc.setflags(write=False)
    return depth, mc


def depth_share(a, b):
    return float((_bits(a) != _bits(b)).mean())


def class_of(d):
    return np.where(np.isnan(d), 0, np.where(np.isposinf(d), 1, np.where(np.isneginf(d), 2, 3)))


def peaks_share(a, b):
    """share of pixels whose (cost, depth) lists differ; the shorter list padded at the front with the empty entry"""
    ka, kb = a.shape[2], b.shape[2]
    k = max(ka, kb)

    def pad(p):
        out = np.zeros(p.shape[:2] + (k, 2))
        out[..., 1] = -1.0
        out[:, :, k - p.shape[2]:] = p
        return out
    return float((_bits(pad(a)) != _bits(pad(b))).any(axis=(2, 3)).mean())


def measured_share(e):
    """what the entry's witness measures on the oracle, against the same case at the default constants"""
    d = default_entry(e.case)
    if e.witness == "depth":
        if e.case.startswith("mvs"):
            return depth_share(oracle_mvs(e, 0)[0], oracle_mvs(d, 0)[0])
        return depth_share(oracle_twoview(e, 0)[0], oracle_twoview(d, 0)[0])
    if e.witness == "sad":
        return depth_share(oracle_sad(e, 0)[0], oracle_sad(d, 0)[0])
    if e.witness == "peaks":
        return peaks_share(oracle_mvs(e, 0)[1], oracle_mvs(d, 0)[1])
    if e.witness == "cross":
        got, want = oracle_cross(e), oracle_cross(d)
        return float(np.mean([(class_of(g) != class_of(w)).mean() for g, w in zip(got, want)]))
    raise KeyError(e.witness)
