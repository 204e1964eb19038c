"""The DAE's building blocks at their edges: the DeGrooteFregly2016 curves and
muscle, the SimmSpline evaluators and the piecewise-polynomial tables of
csrc/dae_device.hpp against tests/_dae_edges_ref.py, a long-double restatement
with a counted bound e per value.  Everywhere |got - reference| <= e, entry by
entry; ``got`` is the device's (tests marked gpu) or the CPU oracle's (the
unmarked tests, which also hold the reference to its own properties).

A  the muscle on the slider (L = height, S = its speed): all 34 outputs and
   what dgf_eval hands the DAE, rows built backwards from curve targets.
B  the SimmSpline through the coupled pendulum's CoordinateCoupler with
   implicit dynamics: the kinematic-error and velocity-correction outputs are
   closed forms of the spline's value, slope and curvature.
C  tables through prescribed kinematics on the slider: value, first and second
   derivative on breaks, one ulp either side and past the ends.
D  gait10dof18musc_inverse and gait10dof18musc, generated against generic, on
   table breaks and spline knots, and with jittered table times (the
   direct-index segment search of the ground-reaction table).

Each comparison prints its max err / e ("dae_edges ..." lines, pytest -s)."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

import _dae_edges_ref as R
from _dae_edges_ref import B
from _objective_ref import EPS, LD, Layout
from mocohip import abi, configs
from mocohip.model import DataTable, Function
from test_muscle_outputs import SLIDER, _hip, restated_outputs

NAMES = list(abi.MUSCLE_OUTPUTS)
PATH = "/forceset/actuator"
MASS, GRAVITY = configs.HANGING_MUSCLE_MASS, configs.HANGING_MUSCLE_GRAVITY


def _report(label, r):
    """Print and return the largest err / e of a comparison."""
    m = float(np.max(r, initial=0.0))
    print(f"dae_edges {label}: max err / e = {m:.3g}")
    return m


def _within(label, got, want: B, where=None):
    r = R.ratio(got, want)
    m = _report(label, r)
    if m > 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
        w = where(i) if where else i
        raise AssertionError(f"{label}: err / e = {m:.3g} at {w}: got {np.asarray(got)[i]!r}, "
                             f"reference {float(want.v[i])!r} +- {float(want.e[i]):.3g}")
    return m


def _oracle(st):
    from mocohip.solver import OracleNLP
    return OracleNLP(st.problem.create_rep(), st.solver.options())


def _backend_for(st):
    lib = abi.load_mocohip()
    rep, opts = st.problem.create_rep(), st.solver.options()
    buf = C.create_string_buffer(128)
    assert lib.mh_backend_for(C.byref(rep.struct), C.byref(opts), buf, 128) == 0, lib.mh_last_error()
    return buf.value.decode()


# ==== A: the muscle on the slider =====================================================

ACT_EXC = [(0.01, 0.0), (0.5, 1.0), (1.0, 1.0), (0.5, 0.5), (1.0, 0.0), (0.01, 1.0)]   # (two with exc == act)
EXC_ALONE = [0.01, 0.5, 1.0, 0.0]            # a muscle without activation dynamics runs on its excitation
NFV = [-1.5, -1.0, 0.0, 1e-9, 1.0, 1.5]
LENGTHS = [("nfl", 0.2), ("nfl", 1.0), ("nfl", 1.8), ("along", 1e-4), ("along", 1e-5)]
NEGATIVE = ("along", -1e-3)                  # rigid tendon only: the insertion behind the tendon's end
FTN = [0.0, 1.0, 5.0]
DFT = [-50.0, 0.0, 50.0]
FV = [0.0, -1e-3, 1.0, 1.794, 2.5]
SPEEDS = [-0.2, 0.0, 0.15]
SIZES = {"rigid": 6 * 6 * 6, "rigid_no_activation_dynamics": 6 * 4 * 6, "rigid_no_passive_force": 6 * 6 * 6,
         "compliant_explicit": 5 * 3 * 5 * 3 + 3 * 3, "compliant_implicit": 5 * 3 * 3 * 3 * 6}


class Slider:
    """One variant of the hanging muscle: the study, its layout, the muscle's
    data, where each input sits in a row and each derivative in eval_dae's
    output, and the rows."""

    def __init__(self, variant):
        self.variant = variant
        self.st = configs.hanging_muscle(2, **SLIDER[variant])
        self.rep = self.st.problem.create_rep()
        self.lay = Layout(self.rep, self.st.solver.options())
        self.M = R.Muscle(self.rep, 0)
        sn, cn = self.rep.state_names, self.rep.control_names
        assert sn[:2] == ["/jointset/joint/height/value", "/jointset/joint/height/speed"] and cn == [PATH]
        NS, NC = len(sn), len(cn)
        find = lambda n: sn.index(PATH + n) if PATH + n in sn else -1   # noqa: E731
        self.sa, self.sf = find("/activation"), find("/normalized_tendon_force")
        self.ic = NS
        self.idf = NS + NC if self.M.implicit_tendon else -1
        assert self.lay.NI == NS + NC + (1 if self.idf >= 0 else 0)
        assert (self.sa >= 0) == self.M.has_act and (self.sf >= 0) == (not self.M.rigid)
        self.NZ = NS - 2
        self.rows = self._rows()

    # -- rows, built backwards from the targets, in double
    def _geometry(self, kind, x):
        lopt, sqW = self.M.mu.optimal_fiber_length, self.M.derived[1]
        along = math.sqrt((x * lopt) ** 2 - sqW) if kind == "nfl" else x
        fl = math.sqrt(along * along + sqW)
        return along, fl / lopt, along / fl

    def _length(self, kind, x, tl, along):
        """The height that puts the fibre at the target; for a normalized
        fibre length of 1 the neighbouring double at which dgf_outputs' own
        chain (sqrt and quotient correctly rounded, no contraction) gives 1.0
        exactly, where there is one."""
        L = tl + along
        if (kind, x) != ("nfl", 1.0):
            return L
        lopt, sqW = self.M.mu.optimal_fiber_length, self.M.derived[1]
        for k in sorted(range(-256, 257), key=abs):
            Lk = L + k * math.ulp(L)
            flat = np.float64(Lk) - np.float64(tl)
            if np.sqrt(flat * flat + np.float64(sqW)) / np.float64(lopt) == 1.0:
                return float(Lk)
        return L

    def _tendon(self, ftn, dft=0.0):
        """(tendon length, tendon velocity) in double."""
        kT, lts = self.M.derived[3], self.M.mu.tendon_slack_length
        nTL = math.log(R.INV_C1 * (ftn + R.C3)) / kT + R.C2
        return lts * nTL, lts * (dft / (R.C1 * kT * math.exp(kT * (nTL - R.C2))))

    def _rows(self):
        M, mu = self.M, self.M.mu
        vmax, lts = M.derived[2], mu.tendon_slack_length
        rows = []   # (q, u, act, exc, ftn, dft)
        if M.rigid:
            pairs = ACT_EXC if M.has_act else [(e, e) for e in EXC_ALONE]
            for (kind, x), (act, exc), nfv in itertools.product(LENGTHS + [NEGATIVE], pairs, NFV):
                along, _, cos = self._geometry(kind, x)
                rows.append((self._length(kind, x, lts, along), nfv * vmax / cos, act, exc, 0.0, 0.0))
        elif M.implicit_tendon:
            for (kind, x), ftn, dft, (act, exc), nfv in itertools.product(LENGTHS, FTN, DFT, ACT_EXC[:3], NFV):
                along, _, cos = self._geometry(kind, x)
                tl, tv = self._tendon(ftn, dft)
                S = 0.0 if (nfv == 0.0 and dft == 0.0) else nfv * vmax / cos + tv
                rows.append((self._length(kind, x, tl, along), S, act, exc, ftn, dft))
        else:
            fal = lambda l: float(R.dgf_fal(mu.active_force_width_scale, B.of(l)).v)   # noqa: E731
            fpe = lambda l: float(R.dgf_fpe(M, B.of(l)).v)   # noqa: E731
            for (kind, x), (act, exc), fV, S in itertools.product(LENGTHS, ACT_EXC[:3], FV, SPEEDS):
                along, nfl, cos = self._geometry(kind, x)
                ftn = cos * (fV * act * fal(nfl) + fpe(nfl))
                rows.append((self._tendon(ftn)[0] + along, S, act, exc, ftn, 0.0))
            for ftn, S in itertools.product(FTN, SPEEDS):   # (full activation: the curve's argument stays small)
                along, _, _ = self._geometry("nfl", 1.0)
                rows.append((self._tendon(ftn)[0] + along, S, 1.0, 1.0, ftn, 0.0))
        return np.array(rows, float)

    def inputs(self):
        q, u, act, exc, ftn, dft = self.rows.T
        X = np.zeros((len(self.rows), 1 + self.lay.NI))
        X[:, 1], X[:, 2], X[:, 1 + self.ic] = q, u, exc
        if self.sa >= 0:
            X[:, 1 + self.sa] = act
        if self.sf >= 0:
            X[:, 1 + self.sf] = ftn
        if self.idf >= 0:
            X[:, 1 + self.idf] = dft
        return X

    def reference(self, mutation=None):
        q, u, act, exc, ftn, dft = self.rows.T
        L, S = R.slider_path(q, u)
        out = R.muscle(self.M, L, S, act, exc, ftn, dft, mutation)
        out["udot"] = R.slider_udot(MASS, GRAVITY, out["tendon_force"], q)
        return out

    def dae_columns(self):
        """eval_dae's outputs: udot, the states' derivatives in state order,
        the implicit tendon's residual."""
        cols = {"udot": 0}
        if self.sa >= 0:
            cols["adot"] = 1 + self.sa - 2
        if self.sf >= 0:
            cols["ftdot"] = 1 + self.sf - 2
        if self.idf >= 0:
            cols["residual"] = 1 + self.NZ
        return cols

    def where(self, names):
        return lambda i: (dict(zip(("q", "u", "act", "exc", "ftn", "dft"), self.rows[i[0]])), names[i[1]])


@functools.lru_cache(maxsize=None)
def _slider(variant):
    return Slider(variant)


def _check_dae(label, s, got, ref):
    cols = s.dae_columns()
    assert got.shape == (len(s.rows), 1 + s.NZ + (1 if s.idf >= 0 else 0))
    names = list(cols)
    want = B(np.stack([ref[n].v for n in names], 1), np.stack([ref[n].e for n in names], 1))
    return _within(label, got[:, [cols[n] for n in names]], want, s.where(names))


def _check_outputs(label, s, got, ref):
    assert got.shape == (len(s.rows), 34)
    want = B(np.stack([ref[n].v for n in NAMES], 1), np.stack([ref[n].e for n in NAMES], 1))
    return _within(label, got, want, s.where(NAMES))


def _check_exact_zeros(s, got_out, got_dae):
    """What must be 0.0 exactly: adot where the excitation is the activation
    bit for bit; the tendon strain at zero tendon force; a rigid tendon's
    strain and velocity."""
    q, u, act, exc, ftn, dft = s.rows.T
    if s.sa >= 0 and got_dae is not None:
        same = act == exc
        assert same.any() and (got_dae[same, s.dae_columns()["adot"]] == 0.0).all()
    if got_out is not None:
        slack = np.ones(len(q), bool) if s.M.rigid else ftn == 0.0
        assert slack.any() and (got_out[slack, NAMES.index("tendon_strain")] == 0.0).all()
        if s.M.rigid:
            assert (got_out[:, NAMES.index("tendon_velocity")] == 0.0).all()


def _oracle_outputs(s):
    """All 34 outputs from the oracle's curves: test_muscle_outputs'
    restatement (double arithmetic around orc_dgf_curve) at the slider's own
    L = q and S = (q u) / q."""
    mu = s.rep.compiled._muscles[0]
    out = []
    for q, u, act, exc, ftn, dft in s.rows:
        S = float(np.float64(q) * np.float64(u) / np.float64(abs(q)))
        out.append(restated_outputs(mu, abs(q), S, act if s.sa >= 0 else exc, exc, ftn, dft))
    return np.array(out)


@pytest.mark.parametrize("variant", list(SLIDER))
def test_slider_rows_hit_their_targets(variant):
    """The row-building conditions: the full table, every reference value
    finite, the argument of sinh within +-30; the targets themselves where
    double arithmetic reaches them exactly."""
    s = _slider(variant)
    assert len(s.rows) == SIZES[variant]
    ref = s.reference()
    for n, b in ref.items():
        assert np.isfinite(b.v.astype(float)).all() and np.isfinite(b.e.astype(float)).all(), n
    assert (np.abs(ref["sinh_argument"].v) <= 30).all()
    q, u, act, exc, ftn, dft = s.rows.T
    nfl, nfv = ref["normalized_fiber_length"].v, ref["normalized_fiber_velocity"].v
    for kind, x in LENGTHS:
        v = nfl if kind == "nfl" else ref["fiber_length_along_tendon"].v
        assert (np.abs(v - x) <= 1e-9 * abs(x)).any(), (kind, x)
    assert (ref["cos_pennation_angle"].v.min() < 1.1e-3)
    if s.M.rigid:
        flat = q - s.M.mu.tendon_slack_length               # dgf_outputs' own double chain (no contraction)
        chain = np.sqrt(flat * flat + s.M.derived[1]) / s.M.mu.optimal_fiber_length
        assert (chain == 1.0).sum() == len(s.rows) // 6     # exactly 1, a sixth of the rows
        assert (ref["fiber_length_along_tendon"].v < 0).sum() == len(s.rows) // 6
        assert (nfv == 0.0).sum() == len(s.rows) // 6
    if s.M.rigid or s.M.implicit_tendon:
        for x in NFV:
            assert (np.abs(nfv - x) <= 1e-9 * abs(x) + (1e-20 if x else 0)).any(), x
    else:
        fV = ref["force_velocity_multiplier"].v
        for x in FV:
            assert (np.abs(fV - x) <= 1e-6 * max(abs(x), 1e-3)).any(), x
    if s.M.implicit_tendon:
        assert (nfv == 0.0).any()
    if s.sa >= 0:
        assert (act == exc).any() and set(act) == {0.01, 0.5, 1.0} and {0.0, 1.0} <= set(exc)
    if not s.M.rigid:
        assert {0.0, 1.0, 5.0} <= set(ftn)


@pytest.mark.parametrize("variant", list(SLIDER))
def test_slider_oracle_within_the_bounds(variant):
    s = _slider(variant)
    ref = s.reference()
    orc = _oracle(s.st)
    got_dae = orc.eval_dae(s.inputs())
    orc.close()
    _check_dae(f"A {variant} oracle eval_dae", s, got_dae, ref)
    got_out = _oracle_outputs(s)
    _check_outputs(f"A {variant} oracle curves, 34 outputs", s, got_out, ref)
    _check_exact_zeros(s, got_out, got_dae)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(SLIDER))
def test_slider_device_within_the_bounds(variant):
    s = _slider(variant)
    ref = s.reference()
    nlp = _hip(s.st)
    assert nlp.backend()[0].startswith("generic"), nlp.backend()   # dae_eval, whose operations slider_udot counts
    X = s.inputs()
    got_out = nlp.eval_muscle_outputs([0] * 34, list(range(34)), X)
    got_dae = nlp.eval_dae(X)
    nlp.close()
    _check_outputs(f"A {variant} device 34 outputs", s, got_out, ref)
    _check_dae(f"A {variant} device eval_dae", s, got_dae, ref)
    _check_exact_zeros(s, got_out, got_dae)


def test_derived_constants_agree_with_long_double():
    """The six constants of mus_derived are formed in double, as the host
    forms them (the reference implementation's own arithmetic, 1 + e - 1
    included); the long-double value of the same formula is within 4 eps."""
    for variant in SLIDER:
        mu = _slider(variant).rep.compiled._muscles[0]
        d, ld = R.derived_formulas(mu, float), R.derived_formulas(mu, LD)
        for k in range(6):
            assert abs(LD(d[k]) - ld[k]) <= 4 * EPS * abs(ld[k]), (variant, k, d[k], ld[k])
    # gait10dof18musc's muscles (tendon strain 0.049): five of the six likewise.  kT is not: the double
    # 1 + 0.049 - 1 is 0.049 to 1.1e-16 absolute, 2.3e-15 of it (the reference implementation's own
    # value, which the device mirrors on purpose); printed, and recorded in DESIGN.md
    st = configs.gait10dof18musc(1)
    worst = 0.0
    for mu in st.problem.create_rep().compiled._muscles:
        d, ld = R.derived_formulas(mu, float), R.derived_formulas(mu, LD)
        assert all(abs(LD(d[k]) - ld[k]) <= 4 * EPS * abs(ld[k]) for k in (0, 1, 2, 4, 5))
        worst = max(worst, float(abs(LD(d[3]) - ld[3]) / (EPS * abs(ld[3]))))
    print(f"dae_edges derived kT of gait10dof18musc: double against long double {worst:.3g} eps")


def test_reference_curves_known_answers():
    """Moco/Tests/testMocoActuators.cpp:199-220 ("Curve values"), as
    test_oracle.py pins them on the oracle, here on the reference."""
    class Mu:
        passive_fiber_strain_at_one_norm_force = 0.6

    class M:
        mu = Mu
        derived = [0, 0, 0, math.log(6.0) / (1.0 + 0.049 - 1.0), math.exp(4.0 * (0.2 - 1.0) / 0.6), 0]
    M.derived[5] = math.exp(4.0) - M.derived[4]
    f = lambda b: float(b.v)   # noqa: E731
    assert f(R.tendon_length(M, 0.0)) == pytest.approx(1.0, abs=1e-15)        # f_T(1) == 0, inverted
    assert f(R.tendon_length(M, 1.0)) == pytest.approx(1 + 0.049, rel=1e-10)  # f_T(1 + eps_T) == 1
    assert f(R.dgf_fpe(M, B.of(1.0))) == pytest.approx(0.0182288, rel=1e-4)
    assert f(R.dgf_fpe(M, B.of(0.2))) == pytest.approx(0, abs=1e-4)
    assert f(R.dgf_fpe(M, B.of(1.6))) == pytest.approx(1, rel=1e-4)
    assert f(R.dgf_fal(1.0, B.of(1.0))) == pytest.approx(1)
    assert abs(f(R.dgf_fv(B.of(-1.0)))) < 1e-15
    assert f(R.dgf_fv(B.of(0.0))) == pytest.approx(1)
    assert f(R.dgf_fv(B.of(1.0))) == pytest.approx(1.794, rel=1e-3)
    assert f(R.dgf_fv_inv(R.dgf_fv(B.of(0.37)))) == pytest.approx(0.37, rel=1e-12)
    # the cancellation the counted bound is there for: 17 units cancel in tv + sqrt(tv tv + 1) at v = +1
    b = R.dgf_fv(B.of(1.0))
    assert 10 * EPS * abs(b.v) < b.e < 200 * EPS * abs(b.v)


# ==== B: the SimmSpline through a coupler =============================================

def _coupled(knots=None):
    st = configs.double_pendulum_coupled(1, dynamics="implicit", coupler="spline")
    if knots is not None:
        xs = np.asarray(knots, float)
        st.problem.model.constraints[0].function = Function.simm_spline(
            "q0", xs, -2.0 * xs + math.pi + 0.1 * xs * xs)
    return st


KNOTS = {"13": None, "2": [-1.0, 2.0], "3": [-1.0, 0.5, 2.0]}


class Coupler:
    def __init__(self, which):
        self.st = _coupled(KNOTS[which])
        self.rep = self.st.problem.create_rep()
        self.lay = Layout(self.rep, self.st.solver.options())
        assert self.rep.state_names == ["/jointset/j0/q0/value", "/jointset/j1/q1/value",
                                        "/jointset/j0/q0/speed", "/jointset/j1/q1/speed"]
        # [t | q0 q1 u0 u1 | tau0 tau1 | udot0 udot1 | lambda | gamma]
        assert (self.lay.NI, self.lay.NS, self.lay.NC, self.lay.NDV, self.lay.NM, self.lay.NSL) == (10, 4, 2, 2, 1, 1)
        ms = self.rep.compiled.struct
        assert ms.nconstraints == 1
        K = ms.constraints[0]
        self.sp = R.Spline(self.rep, int(K.func))
        self.scales = (float(K.scale), self.sp.scale)
        assert self.sp.coord == 0 and int(K.dependent) == 1 and self.sp.n == int(which)
        self.rows = self._rows()

    def _rows(self):
        x = self.sp.x
        q0 = []
        for k in x:
            q0 += [np.nextafter(k, -np.inf), k, np.nextafter(k, np.inf)]
        for end in (x[0], x[-1]):
            for w in (1e-13, 2e-13, 3e-13):
                q0 += [end - w, end + w]
        q0 += [x[0] - 0.5, x[-1] + 1.0, -100.0, 100.0, 0.5 * (x[0] + x[1]), 0.5 * (x[-2] + x[-1]) + 0.01]
        if self.sp.n == 13:
            assert -6.5 in q0 and 7.0 in q0
        n = len(q0)
        cyc = lambda vals: np.array([vals[i % len(vals)] for i in range(n)])   # noqa: E731
        X = np.zeros((n, 11))
        X[:, 0] = 0.25
        X[:, 1] = q0
        X[:, 2] = cyc([0.3, -0.8, 1.9])
        X[:, 3] = cyc([0.7, -1.3, 0.0, 2.1])          # (one speed exactly 0)
        X[:, 4] = cyc([-0.4, 0.9, 1.7, -2.2, 0.6])
        X[:, 5], X[:, 6] = 0.1, -0.2
        X[:, 7] = cyc([3.0, -2.0, 0.5, -7.5, 1.25, 9.0, -0.3])
        X[:, 8] = cyc([-1.5, 4.0, 2.5])
        X[:, 9] = cyc([2.0, -1.0])
        X[:, 10] = cyc([0.6, -0.9, 1.4, -0.2, 3.3, -1.7, 0.8, -2.4, 1.1, 0.4, -0.5])
        assert (X[:, 3] == 0.0).any() and (X[:, 3] > 0).any() and (X[:, 3] < 0).any()
        return X

    def candidates(self, row, mutation=None):
        _, q0, q1, u0, u1, _, _, a0, a1, _, gam = row
        return R.coupler_outputs(self.scales, self.sp.eval(q0, mutation), q0, q1, u0, u1, a0, a1, gam)

    def worst(self, label, got, mutation=None):
        """max over the rows of (min over the admissible expansions of the
        largest err / e among the five outputs).  Outputs 2..4: the position,
        velocity and acceleration errors; 5, 6: the velocity correction."""
        assert got.shape == (len(self.rows), 7)
        worst = []
        for row, g in zip(self.rows, got):
            per = []
            for cand in self.candidates(row, mutation):
                per.append(max(float(R.ratio(g[2 + j], cand[j])) for j in range(5)))
            worst.append(min(per))
        return _report(label, np.array(worst)), int(np.argmax(worst))


@functools.lru_cache(maxsize=None)
def _coupler(which):
    return Coupler(which)


@pytest.mark.parametrize("which", list(KNOTS))
def test_spline_reference_interpolates_its_knots_and_extrapolates_linearly(which):
    c = _coupler(which)
    sp = c.sp
    for k in range(sp.n):
        for v, d1, d2 in sp.eval(sp.x[k]):
            assert abs(v.v - LD(sp.y[k])) <= v.e, (k, v.v, sp.y[k])
    for t, end in ((sp.x[0] - 3.0, 0), (sp.x[-1] + 3.0, sp.n - 1)):
        (v, d1, d2), = sp.eval(t)
        assert d2.v == 0.0 and d2.e == 0.0 and d1.v == LD(sp.b[end]) and d1.e == 0.0
    # either side of the 2e-13 end windows, and on them
    assert sp.segments(sp.x[0] + 1e-13) == [0] and sp.segments(sp.x[-1] - 1e-13) == [sp.n - 1, sp.n - 2]
    assert sp.segments(sp.x[-1] - 3e-13) == [sp.n - 2] and len(sp.eval(sp.x[-1] + 1e-13)) == 1
    if sp.n > 2:
        assert sp.segments(sp.x[1]) == [0, 1] and sp.segments(np.nextafter(sp.x[1], 9.0)) == [1]


@pytest.mark.parametrize("which", list(KNOTS))
def test_spline_oracle_within_the_bounds(which):
    c = _coupler(which)
    orc = _oracle(c.st)
    assert orc.NO == 7
    got = orc.eval_dae(c.rows)
    orc.close()
    m, at = c.worst(f"B {which} knots oracle", got)
    assert m <= 1.0, (m, c.rows[at], got[at])


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(KNOTS))
def test_spline_device_within_the_bounds(which):
    """A spline coupler has no generated back end (generated:coupled_pendulum
    serves the linear coupler with explicit dynamics): the default selection is
    the interpreter, simm_eval's binary search, at 13 knots and at 2 and 3,
    where the search has its corner.  (simm_eval_k, behind the generated
    interval count, runs in test_knee_on_spline_knots_generated_against_generic.)"""
    c = _coupler(which)
    assert _backend_for(configs.double_pendulum_coupled(1)) == "generated:coupled_pendulum"
    nlp = _hip(c.st)
    assert nlp.backend()[0].startswith("generic"), nlp.backend()
    got = nlp.eval_dae(c.rows)
    nlp.close()
    m, at = c.worst(f"B {which} knots device", got)
    assert m <= 1.0, (m, c.rows[at], got[at])


# ==== C: tables through prescribed kinematics =========================================

def _heights(n, seed):
    r = np.random.default_rng(seed)
    t = np.cumsum(r.uniform(7.0, 13.0, n)) - 5.0       # unequal spacing, ~10 s: the end segments
    return t, 0.15 + r.uniform(-0.004, 0.004, n)      # extrapolate 10 s without leaving the muscle's range


TABLES = {"degree5": (5, 9), "degree3": (3, 8), "degree1": (1, 6),
          "degree5_fewest_kept": (5, 6), "degree3_fewest_kept": (3, 4),
          "degree5_fewest": (5, 2), "degree3_fewest": (3, 2), "degree1_fewest": (1, 2)}
FEWEST_ROWS = 2    # gcv_interpolating_ppoly (splines.py): "need at least two samples"; a degree the
#                    rows cannot carry is lowered to the largest odd degree below the row count


def _table_study(name):
    degree, n = TABLES[name]
    t, h = _heights(n, 40 + n + degree)
    st = configs.hanging_muscle(2, dynamics="implicit")
    st.problem.set_position_motion(DataTable("kin", t, {"/jointset/joint/height/value": h}, degree=degree))
    return st


class Prescribed:
    def __init__(self, name):
        self.st = _table_study(name)
        self.rep = self.st.problem.create_rep()
        self.lay = Layout(self.rep, self.st.solver.options())
        assert self.rep.state_names == [PATH + "/activation"] and self.lay.NI == 2
        self.tab = R.Table(self.rep, "__position_motion")
        degree, n = TABLES[name]
        assert self.tab.nseg == n - 1 and self.tab.ncol == 1
        assert self.tab.degree == min(degree, n - 1 if (n - 1) % 2 else n - 2)
        self.M = R.Muscle(self.rep, 0)
        br = self.tab.br
        t = []
        for b in br:
            t += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
        t += [br[0] - 0.1, br[-1] + 0.1, br[0] - 10.0, br[0] + 10.0, br[-1] - 10.0, br[-1] + 10.0]
        mid = self.tab.nseg // 2
        t += [0.5 * (br[0] + br[1]), 0.5 * (br[mid] + br[mid + 1]), 0.5 * (br[-2] + br[-1])]
        self.t = np.array(t)
        n = len(t)
        self.X = np.column_stack([self.t, np.resize([0.3, 0.8, 0.05], n), np.resize([0.6, 0.1], n)])

    def reference(self, mutation=None):
        q, u, a = self.tab.eval(0, self.t, mutation)
        L, S = R.slider_path(q, u)
        out = R.muscle(self.M, L, S, self.X[:, 1], self.X[:, 2], 0.0, 0.0)
        out["residual"] = R.slider_residual(MASS, GRAVITY, out["tendon_force"], q, a)
        for n, b in out.items():
            assert np.isfinite(b.v.astype(float)).all() and np.isfinite(b.e.astype(float)).all(), n
        assert (out["normalized_fiber_length"].v > 0.3).all() and (out["normalized_fiber_length"].v < 1.9).all()
        return out

    def check_dae(self, label, got, ref):
        assert got.shape == (len(self.t), 2)
        want = B(np.stack([ref["residual"].v, ref["adot"].v], 1), np.stack([ref["residual"].e, ref["adot"].e], 1))
        return _within(label, got, want, lambda i: (self.t[i[0]], ("residual", "adot")[i[1]]))


@functools.lru_cache(maxsize=None)
def _prescribed(name):
    return Prescribed(name)


def test_table_fit_refuses_one_row_below_the_fewest():
    assert FEWEST_ROWS == 2
    for degree in (1, 3, 5):
        st = configs.hanging_muscle(2, dynamics="implicit")
        st.problem.set_position_motion(DataTable("kin", np.array([0.5]), {"/jointset/joint/height/value":
                                                                         np.array([0.15])}, degree=degree))
        with pytest.raises(ValueError, match="need at least two samples"):
            st.problem.create_rep()


@pytest.mark.parametrize("name", list(TABLES))
def test_table_reference_returns_the_new_segment_s_constant_term_at_a_break(name):
    p = _prescribed(name)
    tab = p.tab
    v, d1, d2 = tab.eval(0, tab.br[:-1])
    # (dt = 0 exactly; what is left of the bound is the eps |v| of the additions of 0 the value passes
    # through: one for the value, two for the slope)
    assert (v.v == tab.cf[:, 0, 0]).all() and (v.e <= EPS * np.abs(v.v)).all()
    assert (d1.v == tab.cf[:, 0, 1]).all() and (d1.e <= 2 * EPS * np.abs(d1.v)).all()
    assert list(tab.segment(tab.br)) == list(range(tab.nseg)) + [tab.nseg - 1]
    assert list(tab.segment(np.nextafter(tab.br, -np.inf))) == [0] + list(range(tab.nseg))
    assert list(tab.segment([tab.br[0] - 10, tab.br[-1] + 10])) == [0, tab.nseg - 1]
    if name == "degree1":   # unequal slopes: the speed jumps at every interior break
        assert (np.diff(tab.cf[:, 0, 1]) != 0.0).all()


@pytest.mark.parametrize("name", list(TABLES))
def test_table_oracle_within_the_bounds(name):
    p = _prescribed(name)
    ref = p.reference()
    orc = _oracle(p.st)
    got = orc.eval_dae(p.X)
    orc.close()
    p.check_dae(f"C {name} oracle eval_dae", got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLES))
def test_table_device_within_the_bounds(name):
    p = _prescribed(name)
    ref = p.reference()
    nlp = _hip(p.st)
    got_dae = nlp.eval_dae(p.X)
    got_ls = nlp.eval_muscle_outputs([0, 0], [0, 1], p.X)
    nlp.close()
    want = B(np.stack([ref["length"].v, ref["lengthening_speed"].v], 1),
             np.stack([ref["length"].e, ref["lengthening_speed"].e], 1))
    _within(f"C {name} device length, speed", got_ls, want, lambda i: (p.t[i[0]], i[1]))
    p.check_dae(f"C {name} device eval_dae", got_dae, ref)


# ==== sensitivity: the reference mutated, one change at a time ========================

def _dae_ratio(s, got, ref):
    cols = s.dae_columns()
    names = list(cols)
    want = B(np.stack([ref[n].v for n in names], 1), np.stack([ref[n].e for n in names], 1))
    return R.ratio(got[:, [cols[n] for n in names]], want)


def _violations(open_nlp, side):
    """Per mutation the largest err / e of ``side``'s eval_dae against the
    mutated reference (the violation factor), after the same values passed
    the reference as it stands."""
    out = {}
    for mutation, variant in (("fal_constant", "rigid"), ("no_passive_offset", "rigid"),
                              ("no_d3", "compliant_explicit")):
        s = _slider(variant)
        nlp = open_nlp(s.st)
        got = nlp.eval_dae(s.inputs())
        nlp.close()
        assert _dae_ratio(s, got, s.reference()).max() <= 1.0
        out[mutation] = float(_dae_ratio(s, got, s.reference(mutation)).max())
    p = _prescribed("degree1")
    nlp = open_nlp(p.st)
    got = nlp.eval_dae(p.X)
    nlp.close()
    for mutation in (None, "old_segment"):
        ref = p.reference(mutation)
        r = R.ratio(got, B(np.stack([ref["residual"].v, ref["adot"].v], 1),
                           np.stack([ref["residual"].e, ref["adot"].e], 1)))
        if mutation is None:
            assert r.max() <= 1.0
        else:
            out[mutation] = float(r.max())
            on_break = np.isin(p.t, p.tab.br[1:-1])
            assert (r[on_break].max(1) > 1.0).all() and (r[~on_break] <= 1.0).all()   # the interior breaks, only
    c = _coupler("13")
    nlp = open_nlp(c.st)
    got = nlp.eval_dae(c.rows)
    nlp.close()
    assert c.worst(f"B 13 knots {side}", got)[0] <= 1.0
    out["neighbour_slope"] = c.worst(f"B 13 knots {side}, extrapolation slope of the neighbouring knot", got,
                                     "neighbour_slope")[0]
    for mutation, v in out.items():
        print(f"dae_edges mutation {mutation} on the {side}'s values: violation factor {v:.3g}")
    assert len(out) == 5 and all(v > 1.0 for v in out.values()), out
    return out


def test_mutations_rejected_on_the_oracle():
    _violations(_oracle, "oracle")


@pytest.mark.gpu
def test_mutations_rejected_on_the_device():
    _violations(_hip, "device")


# ==== D: generated against generic on breaks and knots ================================

JITTER = 0.3    # of the spacing; match() accepts it (test_jittered_tables_keep_the_generated_back_end)


def _jittered(jitter=JITTER):
    """gait10dof18musc_inverse with the times of its kinematics table and of
    its ground-reaction table moved, deterministically, by up to +-jitter of
    the spacing (the ends stay).  The ground-reaction table is the one the
    generated code searches by direct index (codegen.py external_forces)."""
    st = configs.gait10dof18musc_inverse(1)
    r = np.random.default_rng(77)
    for tab in (st.problem.position_motion, st.problem.model.tables["grf"]):
        t = np.asarray(tab.times, float).copy()
        h = (t[-1] - t[0]) / (len(t) - 1)
        d = r.uniform(-jitter, jitter, len(t)) * h
        d[::2], d[1::2] = -np.abs(d[::2]), np.abs(d[1::2])     # alternate early / late: both corrections occur
        d[0] = d[-1] = 0.0
        tab.times = t + d
        assert (np.diff(tab.times) > 0).all()
    return st


def _direct_guess(br, t):
    """table_segment_ur's first guess (dae_device.hpp:1294-1295) with the
    generator's 1 / spacing (codegen.py _uniform_guess)."""
    n = len(br) - 1
    inv = n / (br[-1] - br[0])
    return np.clip(((t - br[0]) * inv).astype(int), 0, n - 1)


def _edge_times(br, lo, hi):
    """Every break, one ulp either side, and the middle of every segment,
    within [lo, hi]."""
    t = np.concatenate([np.nextafter(br, -np.inf), br, np.nextafter(br, np.inf), 0.5 * (br[:-1] + br[1:])])
    return np.sort(t[(t >= lo) & (t <= hi)])


def test_jittered_tables_keep_the_generated_back_end():
    """match() accepts the jitter used, and the direct guess is then wrong by
    one in both directions (and right elsewhere), so that both branches of the
    correction step run."""
    assert _backend_for(_jittered()) == "generated:gait10dof18musc_inverse"
    rep = _jittered().problem.create_rep()
    tab = R.Table(rep, "grf")
    t = _edge_times(tab.br, tab.br[0], tab.br[-1])
    off = _direct_guess(tab.br, t) - tab.segment(t)
    assert set(off) == {-1, 0, 1}, set(off)
    assert (off == -1).sum() > 100 and (off == 1).sum() > 100
    # the bundled table: the guess is nearly always right
    tab0 = R.Table(configs.gait10dof18musc_inverse(1).problem.create_rep(), "grf")
    t0 = _edge_times(tab0.br, tab0.br[0], tab0.br[-1])
    print("dae_edges D direct guess off by one: bundled grf table", float((_direct_guess(tab0.br, t0) !=
          tab0.segment(t0)).mean()), "jittered", float((off != 0).mean()))


def _inverse_rows(nlp, times):
    from test_muscle_outputs import _grid_rows, _muscle_range
    x = _muscle_range(nlp, np.random.default_rng(5))
    base = _grid_rows(nlp, x)[1]
    rows = np.tile(base, (len(times), 1))
    rows[:, 0] = times
    return rows


def _dae_against_oracle(label, st, rows_of):
    """eval_dae of both back ends against the oracle at the project's margin
    (test_gpu_parity's row scale, test_muscle_outputs' TOL); returns the two
    contexts' outputs 0 and 1 of all muscles."""
    from test_gpu_parity import _assert_close, _scale
    from test_muscle_outputs import TOL
    orc = _oracle(st)
    nm = len(st.problem.model.muscles)
    mus = [im for im in range(nm) for _ in (0, 1)]
    ls = []
    rows = Y0 = None
    for generic in (False, True):
        nlp = _hip(st, generic)
        name = nlp.backend()[0]
        assert name.startswith("generic") if generic else name.startswith("generated:"), name
        if rows is None:
            rows = rows_of(nlp)
            Y0 = orc.eval_dae(rows)
        Y = nlp.eval_dae(rows)
        tol = TOL * (_scale(Y0).max(1, keepdims=True) + 1.0)
        fin = np.isfinite(Y0)
        print(f"dae_edges {label} {name}: max |d| / tol = {float((np.abs(Y - Y0)[fin] / np.broadcast_to(tol, Y0.shape)[fin]).max()):.3g}"
              f" over {len(rows)} rows")
        _assert_close(Y, Y0, tol)
        ls.append(nlp.eval_muscle_outputs(mus, [0, 1] * nm, rows))
        nlp.close()
    orc.close()
    return rows, ls


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["bundled", "jittered"])
def test_inverse_on_table_breaks_generated_against_generic(table):
    """gait10dof18musc_inverse at times on every break of the kinematics table
    and of the ground-reaction table, one ulp either side, and in the middle
    of every segment (where a segment off by one shows: the neighbour's
    polynomial, extrapolated): outputs 0 and 1 of all 18 muscles bit for bit
    equal between the two contexts, eval_dae of both against the oracle."""
    st = configs.gait10dof18musc_inverse(1) if table == "bundled" else _jittered()
    rep = st.problem.create_rep()
    kin, grf = R.Table(rep, "__position_motion"), R.Table(rep, "grf")
    lo, hi = max(kin.br[0], grf.br[0]), min(kin.br[-1], grf.br[-1])
    times = np.concatenate([_edge_times(kin.br, lo, hi), _edge_times(grf.br, lo, hi)])
    rows, (a, b) = _dae_against_oracle(f"D {table} tables", st, lambda nlp: _inverse_rows(nlp, times))
    assert a.shape == (len(times), 36) and np.array_equal(a, b)


@pytest.mark.gpu
def test_knee_on_spline_knots_generated_against_generic():
    """gait10dof18musc with both knee angles on every knot of every SimmSpline
    that reads a knee angle (knee translations, moving path points), one ulp
    either side and outside the knot range.  eval_dae of the generated back
    end (simm_eval_k behind the generated interval count) and of the
    interpreter (simm_eval) against the oracle; outputs 0 and 1 of all 18
    muscles against the checker of test_muscle_outputs at its TOL, and equal
    bit for bit between the two contexts off the knots."""
    from test_muscle_outputs import TOL, Checker, _grid_rows, _muscle_range
    st = configs.gait10dof18musc(1)
    rep = st.problem.create_rep()
    ms = rep.compiled.struct
    qi = rep.compiled.qidx
    knees = (qi["knee_angle_r"], qi["knee_angle_l"])
    knots = set()
    for f in range(ms.nfunctions):
        F = ms.functions[f]
        if F.kind == abi.MH_FN_SIMMSPLINE and F.coord in knees:
            knots |= {float(ms.knot_x[F.knot_begin + i]) for i in range(F.knot_count)}
    knots = np.array(sorted(knots))
    assert len(knots) >= 17
    angles = np.concatenate([np.nextafter(knots, -np.inf), knots, np.nextafter(knots, np.inf),
                             [knots[0] - 0.1, knots[-1] + 0.1, knots[0] - 2e-13, knots[-1] + 2e-13,
                              knots[0] + 1e-13, knots[-1] - 1e-13]])

    def rows_of(nlp):
        x = _muscle_range(nlp, np.random.default_rng(5))
        x[0], x[1] = 0.3, 1.2
        rows = np.tile(_grid_rows(nlp, x)[1], (len(angles), 1))
        for k in knees:
            rows[:, 1 + k] = angles
        return rows
    rows, (a, b) = _dae_against_oracle("D knee knots", st, rows_of)
    ck = Checker(st)
    want = np.array([[v for im in range(18) for v in ck.length_speed(im, r)] for r in rows])
    ck.orc.close()
    for got in (a, b):
        assert (np.abs(got - want) <= TOL * (np.abs(want) + 1.0)).all()
    off = ~np.isin(angles, knots)
    assert np.array_equal(a[off], b[off])
