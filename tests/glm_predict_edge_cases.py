"""TEST INFRASTRUCTURE ONLY: the launch rule and the case builders of the edge suites of ``loo_glm_predict``.

``tests/test_glm_predict_edges_host.py`` proves, on the NumPy restatement alone, that the shapes below reach the regimes they are
named after and that the builders' inputs make a comparison meaningful (finite references, PIT values strictly inside (0, 1), the
distribution functions scipy's own); ``tests/test_gpu_loo_glm_predict_edges.py`` runs the same inputs through the kernels.  The
inputs are defined here, once.  Pure NumPy / scipy: nothing here imports the package or touches a GPU.

The constants mirror csrc/pla_glm.h, csrc/pla_glm_predict.h and csrc/pla_k_glm_predict.hip: tiles of TILE = 16 observations by 16
draws, a segment of SEG = 16 tiles of draws, kWantWaves = 8192 wavefronts wanted per launch, the row-maximum kernel's cap of 16 384
workgroups of 4 rows and the combine kernel's cap of 8192 workgroups of 256 rows.

PLANTED ROWS.  ``case(family, planted=True)`` writes counts 4096 (the cap itself), 0, 200 and 1 into rows 17, 21, 25 and 29 of a
33-row model: the second tile of observations, and in it the four rows (q + 4 g, q = 1) one lane of the predictive kernel rotates
through its walk, among the small counts the generators draw.  For the log-link families a planted row with y >= 1 has its offset
shifted by ``log(y / exp(mean_s eta))`` so that its mode sits near its count (the row with y = 0 stays as drawn).  For the two
binomial families the rows are (y, trials) = (4096, 4096) -- y = trials at the cap --, (0, 4096), (200, 4096) and (1, 12), each
shifted so that the mean of eta is the link of (y + 1/2) / (trials + 1); a fifth row, 18, carries (4096, 8192): with trials held
to 4096 a count of 4096 is the end of the support, where P(Y <= y) is 1 by definition, so the row whose two PIT values both lie
strictly inside (0, 1) after a walk of 4096 turns needs more trials than that.
"""

import functools
import zlib

import numpy as np
from scipy import special as sp

import glm_families_ref as fam_ref
import glm_predict_ref as ref
import glm_ref

TILE = 16
SEG = ref.SEG
WANT_WAVES = 8192
ROWMAX_GRID, ROWMAX_ROWS = 16384, 4
COMBINE_GRID, COMBINE_ROWS = 8192, 256
FAMILIES = ref.ENGINE_FAMILIES
DISCRETE = ref.DISCRETE
BINOMIAL = ("binomial", "binomial_probit")
# the family as the route text of pla_glm_predict names it
ROUTE_NAME = {"gaussian": "gaussian", "binomial": "binomial logit", "poisson": "poisson log", "negbinomial": "negative binomial log",
              "gamma": "gamma log", "binomial_probit": "binomial probit"}
FIELDS = ("mean", "m2", "pit_le", "pit_lt")

N, S, P = 33, 300, 5
PLANT_LOG = {17: 4096.0, 21: 0.0, 25: 200.0, 29: 1.0}
PLANT_BINOMIAL = {17: (4096.0, 4096.0), 21: (0.0, 4096.0), 25: (200.0, 4096.0), 29: (1.0, 12.0), 18: (4096.0, 8192.0)}
INSIDE_ROWS = {fam: ((25, 18) if fam in BINOMIAL else (25, 17)) for fam in DISCRETE}  # counts 200 and 4096, both PIT values in (0, 1)
CAP_ROW = 17      # the row whose count the cap tests push to 4097 and to -1
PREDICTORS = (5, 17, 40, 100, 129)  # 1, 2, 4, 8 chunks of 16 predictors in registers, then panels of 8
MIXED_DRAWS = (16 * SEG - 1, 16 * SEG + 1, 300)

# (n_rows, n_draws, n_pred) of the large launches, and the row blocks whose separate calls have one segment per wavefront
STRIPS = (8200, 4100, 5)
STRIPS_BLOCKS = ((0, 4100), (4100, 8200))
STRIPS_ROWS = tuple(range(0, 16)) + tuple(range(4096, 4112)) + tuple(range(8192, 8200))
TWO_SEGMENTS = (131080, 272, 3)
TWO_SEGMENTS_BLOCKS = tuple((a, a + 32770) for a in range(0, 131080, 32770))
TWO_SEGMENTS_ROWS = tuple(range(0, 16)) + tuple(range(65536, 65552)) + tuple(range(131072, 131080))
SECOND_ROUNDS = (2097452, 2, 1)
# (family, draws, predictors, planted) -> a salt of the seed: the first draw of these left fewer than half of the rows with both PIT
# values strictly inside (0, 1) (counts of zero have P(Y < y) = 0), a condition on the inputs tests/test_glm_predict_edges_host.py holds
# The Gaussian mean is a weighted sum of eta itself, held to a relative 1e-12 against long double.  Any order of summation is good
# to (S + 4) 2^-53 W(|eta|) only, which is below 1e-12 |W(eta)| where |W(eta)| >= 0.03 W(|eta|) at S = 250: the Gaussian cases carry
# an intercept that keeps eta positive, so the two are equal (the host file asserts the inequality).
GAUSSIAN_SHIFT = 3.0
RESEEDED = {("poisson", 250, 17, False): 1}


def launch_rule(n_rows, n_draws):
    """``(row_tiles, n_seg, strip_segs, n_strips, last_strip_segs)`` of one launch of the predictive kernel:
    ``launch_glm_predict`` in csrc/pla_k_glm_predict.hip, the lines from ``constexpr int64_t kWantWaves = 8192`` to
    ``p.g.n_strips = ...``, with ``glm_predict_segments`` of the same file for ``n_seg``.  A wavefront takes one tile of 16 rows and
    one strip of ``strip_segs`` whole segments (the last strip ``last_strip_segs``)."""
    row_tiles = -(-n_rows // TILE)
    n_seg = -(-(-(-n_draws // TILE)) // SEG)
    strips = min(-(-WANT_WAVES // row_tiles), n_seg)
    strip_segs = -(-n_seg // strips)
    n_strips = -(-n_seg // strip_segs)
    return row_tiles, n_seg, strip_segs, n_strips, n_seg - (n_strips - 1) * strip_segs


def rowmax_rounds(n_rows):
    """Turns of the grid-stride loop of ``glm_predict_rowmax_kernel`` (a wavefront per row, at most 16 384 workgroups of 4)."""
    return -(-n_rows // (ROWMAX_GRID * ROWMAX_ROWS))


def combine_rounds(n_rows):
    """Turns of the grid-stride loop of ``glm_predict_combine_kernel`` (a thread per row, at most 8192 workgroups of 256)."""
    return -(-n_rows // (COMBINE_GRID * COMBINE_ROWS))


def chunks(p):
    """(chunks of 16 predictors, panel route) of ``glm_chunks`` / ``glm_predict_launch_family``."""
    return (1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8), p > 128


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _link(family, p):
    return sp.logit(p) if family == "binomial" else sp.ndtri(p)


@functools.lru_cache(maxsize=None)
def case(family, s=S, p=P, planted=False, n=N):
    """A model of ``glm_ref.make_model`` / ``glm_families_ref.make_model`` with an offset, as a dict of read-only arrays ``X``, ``y``,
    ``beta``, ``scale`` (sigma / phi / alpha or None), ``trials``, ``offset`` and the constants ``oc`` / ``dc`` the fronts hand to
    the engine; ``planted``: the rows of the module's text."""
    rng = np.random.default_rng(seed_of(family, s, p, planted, n) + RESEEDED.get((family, s, p, planted), 0))
    if family in ("gaussian", "binomial", "poisson"):
        m = glm_ref.make_model(rng, n, s, p, family, with_offset=True)
        scale = m["sigma"]
    else:
        m = fam_ref.make_model(rng, n, s, p, family, with_offset=True)
        scale = m["scale"]
    y, offset, trials = m["y"].copy(), m["offset"].copy(), None if m["trials"] is None else m["trials"].copy()
    if family == "gaussian":  # eta of one sign: the weighted mean of eta is then a sum without cancellation (GAUSSIAN_SHIFT)
        y, offset = y + GAUSSIAN_SHIFT, offset + GAUSSIAN_SHIFT
    if planted:
        assert family in DISCRETE and n > max(PLANT_BINOMIAL)
        eta_mean = (m["X"] @ m["beta"].T).mean(axis=1) + offset
        if family in BINOMIAL:
            for r, (yy, nn) in PLANT_BINOMIAL.items():
                y[r], trials[r] = yy, nn
                offset[r] += _link(family, (yy + 0.5) / (nn + 1.0)) - eta_mean[r]
        else:
            for r, yy in PLANT_LOG.items():
                y[r] = yy
                if yy >= 1.0:
                    offset[r] += np.log(yy) - eta_mean[r]
    with np.errstate(all="ignore"):
        oc, dc = ref.constants(family, y, trials, scale)
    return _frozen(dict(family=family, X=m["X"], y=y, beta=m["beta"], scale=scale, trials=trials, offset=offset, oc=oc, dc=dc))


def engine_kwargs(c, put=lambda a: a):
    """The vectors of ``Engine.glm_predict`` for a case."""
    return dict(y=put(c["y"]), offset=put(c["offset"]), trials=put(c["trials"]), obs_const=put(c["oc"]), draw_scale=put(c["scale"]),
                draw_const=put(c["dc"]))


def eta_of(c):
    """NumPy's own linear predictor (the GPU tests take the kernel's)."""
    return glm_ref.linpred(c["X"], c["beta"], c["offset"])


@functools.lru_cache(maxsize=None)
def weights(n, s, seed, minus_inf=0.0):
    """``2 N(0, 1)`` log weights, a share ``minus_inf`` of them log -inf (never a whole row)."""
    rng = np.random.default_rng(seed_of("weights", n, s, seed))
    lw = 2.0 * rng.normal(size=(n, s))
    if minus_inf > 0.0:
        gone = rng.uniform(size=(n, s)) < minus_inf
        gone[:, 0] = False
        lw[gone] = -np.inf
    lw.setflags(write=False)
    return lw


def point(family, eta, y, scale=None, trials=None):
    """``glm_predict_ref.point``, with the rows of large counts walked apart from the others (the restatement walks a whole array as
    many turns as its largest count; the values are per element and do not depend on the company)."""
    y = np.asarray(y, dtype=np.float64)
    big = (y > 64.0) & (y <= ref.MAX_COUNT)
    if family not in DISCRETE or not big.any() or big.all():
        return ref.point(family, eta, y, scale, trials)
    out = [np.empty_like(np.asarray(eta, dtype=np.float64)) for _ in range(4)]
    for rows in (np.flatnonzero(big), np.flatnonzero(~big)):
        part = ref.point(family, eta[rows], y[rows], scale, None if trials is None else np.asarray(trials)[rows])
        for o, a in zip(out, part):
            o[rows] = a
    return tuple(out)


def expected(family, eta, y, scale, trials, lw):
    """``(want, terms)``: the four outputs of FIELDS as the long double weighted sums of the per-element terms on ``eta``, and the
    terms themselves, both as dicts."""
    terms = dict(zip(FIELDS, point(family, eta, y, scale, trials)))
    want = dict(zip(FIELDS, ref.weighted(lw, [terms[f] for f in FIELDS])))
    return want, terms


def fields_of(family):
    return FIELDS[:2] if family == "gamma" else FIELDS


def inside(le, lt):
    """Rows whose two PIT values lie strictly inside (0, 1), P(Y < y) below P(Y <= y)."""
    return (0.0 < lt) & (lt < le) & (le < 1.0)
