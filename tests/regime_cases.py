"""Regime-sweep cases and their metric, shared by tests/test_regime_ref.py (CPU) and
tests/test_regime_gpu.py.  No GPU import.

Medium: template.prm with G = 5, rho = 1, M = 4, dx = 0.01 and group opacities
{1e-6, 1e-2, 1, 1e2, 1e4} / dx, so one handle spans sigma dx over ten decades across its
groups; c dt / dx over eight decades; three boundary pairs; the correction off and on; the
inflow B_g 10^U(-3, 3); two start states (psi = B, and B_g 10^U(-2, 2) per node).

Truth: oracle/fused_np.py (RegionReference on regions) in np.longdouble on the C oracle's fp64
tables -- the answer to "given these fp64 inputs".  Metric, per line (direction i, group g):

    err(x)[i, g] = max over cells and nodes |x - truth| / |truth|

and the code under test must satisfy err(gpu) <= K max(err(oracle_fp64), 16 eps), K = 32:
as close to the truth as the fp64 oracle is, within a small factor, on every line.  The
oracle's own error measures the conditioning of the recurrence at the grid point (3e-16 in
thick cells, 1e-7 for BDF2 at c dt / dx >= 100), so the bound adapts to it.  K: the cell-map
form emulated in fp64 stays within 4.9x of the oracle's error; about 6x headroom for FMA
contraction and the kernels' association.
"""
from collections import namedtuple

import numpy as np

import fused_np
from conftest import PRM_DIR, SEED

K = 32.0
EPS = float(np.finfo(np.float64).eps)
FLOOR = 16.0 * EPS
ORACLE_ERR_MAX = 1e-6        # the fp64 oracle's own line-wise error (a grid point past it would get fewer steps)
TRUTH_RANGE = (1e-250, 1e250)
C_LIGHT = fused_np.C_LIGHT

HAVE_EXTENDED = np.finfo(np.longdouble).nmant >= 63
SKIP_REASON = "np.longdouble has no 64-bit mantissa on this host: no extended-precision truth"

DX = 0.01
G, M = 5, 4
SIGMA_DX = (1e-6, 1e-2, 1.0, 1e2, 1e4)
SCHEMES = (1, 2, 3)
CFL = (1e-4, 1e-2, 1.0, 1e2, 1e4)
BCS = ((1, 1), (2, 1), (0, 0))
VS = (0.0, 5.994)
STARTS = ("B", "random")
STEPS = 6
GRID = [(ts, cfl, bc, V) for ts in SCHEMES for cfl in CFL for bc in BCS for V in VS]
# BDF2 in passes of 20 and 24 steps: 22 and 26 steps, c dt / dx <= 1 (beyond it the reference's
# BDF2 grows the state to 1e49 in 22 steps and the fp64 oracle's own error reaches 1e-3)
LONG_GRID = [(3, cfl, bc, V) for cfl in CFL if cfl <= 1.0 for bc in BCS for V in VS]
LONG_STEPS = (22, 26)

# regions: cells, sigma dx per region (times SIGMA_DX per group), dx, T
REGION_CELLS = ((24, 16, 24), (8, 48, 8))
REGION_SIGMA_DX = (1e-4, 1e3, 1e-2)
REGION_DX = (0.01, 0.04, 0.01)
REGION_T = (1.0, 0.3, 3.0)
REGION_GRID = [(ts, cfl, bc_left, V) for ts in SCHEMES for cfl in CFL for bc_left in (1, 2) for V in VS]

Case = namedtuple("Case", "p q regions ends0 truth oracle mu wt steps")


def to_rt(p):
    return dict(p, bc_left_indicator=p["bc_left"], bc_right_indicator=p["bc_right"])


def _ident(v):
    return f"{v:g}" if isinstance(v, float) else "".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def ids(grid):
    return ["-".join(_ident(v) for v in point) for point in grid]


# ---------------------------------------------------------------------------
# the medium
# ---------------------------------------------------------------------------
_base = {}


def medium(oracle_mod, N, ts, cfl, bc, V, steps=STEPS):
    """The oracle's parameter dict of one grid point, and the tables the truth takes."""
    p = oracle_mod.parse_prm(PRM_DIR / "template.prm", table_dir=PRM_DIR)
    p.update(G=G, M=M, N=N, X=N * DX, rho=1.0, include_validation=0, ts_method=ts, bc_left=bc[0], bc_right=bc[1],
             V=V, use_correction=int(V != 0.0), dt=cfl * DX / C_LIGHT, max_timesteps=steps,
             group_kappa=np.array(SIGMA_DX) / DX, have_group_kappa=1, group_bounds=None, have_group_bounds=0)
    p["dx"] = p["X"] / N
    if "B" not in _base:
        o = oracle_mod.OracleSolver(dict(p, psi_source=np.zeros((M, G))))
        B = o.groups()["B"].copy()
        _base["B"] = B
        _base["psi_source"] = B[None, :] * 10.0 ** np.random.default_rng(SEED).uniform(-3.0, 3.0, size=(M, G))
    p["psi_source"] = _base["psi_source"].copy()
    return p


def start_state(name, N, B=None):
    """None for psi = B (the handle's own start), else B_g 10^U(-2, 2) per node, (M, G, N, 2)."""
    if name == "B":
        return None
    B = _base["B"] if B is None else B
    rng = np.random.default_rng([SEED, N])
    return B[None, :, None, None] * 10.0 ** rng.uniform(-2.0, 2.0, size=(M, G, N, 2))


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------
def line_err(x, truth):
    """(M, G): max over cells and nodes |x - truth| / |truth|."""
    t = np.asarray(truth, dtype=np.longdouble)
    e = np.abs(np.asarray(x, dtype=np.longdouble) - t) / np.abs(t)
    return np.asarray(e.reshape(e.shape[0], e.shape[1], -1).max(axis=2), dtype=np.float64)


def check_conditions(truth, oracle):
    """What keeps a case from passing vacuously; returns the oracle's line-wise error."""
    assert np.isfinite(truth).all() and np.isfinite(oracle).all()
    a = np.abs(truth)
    assert a.min() >= TRUTH_RANGE[0] and a.max() <= TRUTH_RANGE[1], (float(a.min()), float(a.max()))
    err_o = line_err(oracle, truth)
    assert err_o.max() <= ORACLE_ERR_MAX, err_o
    return err_o


def ratio(x, case, groups=slice(None)):
    """(M, G): err(x) / max(err(oracle), 16 eps) per line."""
    truth, oracle = case.truth[:, groups], case.oracle[:, groups]
    err_o = check_conditions(truth, oracle)
    return line_err(x, truth) / np.maximum(err_o, FLOOR)


def check(x, case, groups=slice(None), what=""):
    """The bound on every line; returns the largest ratio."""
    x = np.asarray(x)
    assert np.isfinite(x).all(), what
    r = ratio(x, case, groups)
    assert (r <= K).all(), (what, float(r.max()), np.argwhere(r > K).tolist())
    return float(r.max())


def sequential_moments(psi, mu, wt):
    """phi, F, phi_plus as the reference's sequential sums over the directions (no FMA)."""
    phi = np.zeros(psi.shape[1:])
    F = np.zeros_like(phi)
    pp = np.zeros_like(phi)
    for i in range(psi.shape[0]):
        phi = phi + wt[i] * psi[i]
        F = F + (mu[i] * wt[i]) * psi[i]
        if i >= psi.shape[0] // 2:
            pp = pp + wt[i] * psi[i]
    return phi, F, pp


# ---------------------------------------------------------------------------
# uniform slabs: C oracle against fused_np in extended precision
# ---------------------------------------------------------------------------
class _Truth:
    """fused_np.FusedSolver in np.longdouble for the four (V, start) variants of one
    (N, scheme, c dt / dx, boundary pair) at once: the lines of a FusedSolver are
    independent, so the variants ride as four copies of the groups -- correction off as
    cor1..3 = 0 (every term it adds is then an exact zero), the random start by set_ends.
    Snapshots by step count."""

    def __init__(self, oracle_mod, N, ts, cfl, bc):
        p = medium(oracle_mod, N, ts, cfl, bc, VS[1])
        o = oracle_mod.OracleSolver(p)
        g, c = o.groups(), o.correction_coeffs()
        self.mu, self.wt = o.quad()
        nv = len(VS) * len(STARTS)
        tile = lambda a: np.tile(a, nv)  # noqa: E731
        cor = [np.concatenate([(c[k] if V else np.zeros(G)) for V in VS for _ in STARTS])
               for k in ("cor1", "cor2", "cor3")]
        self.f = fused_np.FusedSolver(dict(p, G=nv * G), self.mu, tile(g["B"]), tile(g["kappa"]), *cor,
                                      np.tile(o.psi_source(), (1, nv)), dtype=np.longdouble)
        ends = self.f.ends()
        rnd = start_state("random", N)
        for v in range(nv):
            if STARTS[v % len(STARTS)] == "random":
                ends[:, v * G:(v + 1) * G] = rnd
        self.f.set_ends(ends)
        self.done = 0
        self.snap = {}

    def at(self, steps, V, start):
        if steps not in self.snap:
            assert steps > self.done, "ask for the step counts in ascending order"
            while self.done < steps:
                self.f.step()
                self.done += 1
            self.snap[steps] = self.f.ends()
        v = VS.index(V) * len(STARTS) + STARTS.index(start)
        return self.snap[steps][:, v * G:(v + 1) * G]


_truths, _cases = {}, {}


def uniform_case(oracle_mod, N, ts, cfl, bc, V, start, steps=STEPS):
    """One grid point with its truth and the C oracle's result, computed once."""
    key = (ts, cfl, bc, V, start, N, steps)
    if key not in _cases:
        tk = (N, ts, cfl, bc)
        if tk not in _truths or (steps not in _truths[tk].snap and steps <= _truths[tk].done):
            _truths[tk] = _Truth(oracle_mod, N, ts, cfl, bc)
        t = _truths[tk]
        p = medium(oracle_mod, N, ts, cfl, bc, V, steps)
        ends0 = start_state(start, N)
        orc = oracle_mod.OracleSolver(p)
        if ends0 is not None:
            orc.set_ends(ends0)
        orc.solve()
        _cases[key] = Case(p, to_rt(p), None, ends0, t.at(steps, V, start), orc.ends(), t.mu, t.wt, steps)
    return _cases[key]


def direct_truth(oracle_mod, case):
    """The truth of one case by a FusedSolver of its own (the check on _Truth's batching)."""
    o = oracle_mod.OracleSolver(case.p)
    g, c = o.groups(), o.correction_coeffs()
    f = fused_np.FusedSolver(case.p, case.mu, g["B"], g["kappa"], c["cor1"], c["cor2"], c["cor3"], o.psi_source(),
                             dtype=np.longdouble)
    if case.ends0 is not None:
        f.set_ends(case.ends0)
    for _ in range(case.steps):
        f.step()
    return f.ends()


# ---------------------------------------------------------------------------
# regions: RegionReference in fp64 against itself in extended precision
# ---------------------------------------------------------------------------
def region_case(oracle_mod, cells, ts, cfl, bc_left, V, start, steps=STEPS):
    """Three regions of sigma dx = REGION_SIGMA_DX x SIGMA_DX, dx and T differing; c dt / dx is
    that of the finest cells."""
    from regions_reference import RegionReference
    key = ("regions", cells, ts, cfl, bc_left, V, start, steps)
    if key not in _cases:
        N = int(sum(cells))
        p = medium(oracle_mod, N, ts, cfl, (bc_left, 1), V, steps)
        widths = [c * d for c, d in zip(cells, REGION_DX)]
        p["X"] = float(sum(widths))
        p["dx"] = p["X"] / N
        regions = [dict(cells=int(c), width=float(w), rho=1.0, kappa_grey=p["kappa_grey"], T=float(T),
                        group_kappa=s * np.array(SIGMA_DX) / d)
                   for c, w, s, d, T in zip(cells, widths, REGION_SIGMA_DX, REGION_DX, REGION_T)]
        ends0 = start_state(start, N)
        out = []
        for dtype in (np.longdouble, np.float64):
            ref = RegionReference(oracle_mod, p, regions, g_lo=0, g_hi=G, dtype=dtype)
            if ends0 is not None:
                ref.set_ends(ends0)
            for _ in range(steps):
                ref.step()
            out.append(ref.ends())
        _cases[key] = Case(p, to_rt(p), regions, ends0, out[0], out[1], ref.mu, ref.wt, steps)
    return _cases[key]
