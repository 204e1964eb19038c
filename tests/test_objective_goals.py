"""The objective kernels (goal_integrand, k_integrand<Z>, k_grad<Z>,
k_reduce_obj, k_marker_final) against the long-double restatement of
tests/_objective_ref.py, at the goal kinds, weights, sizes and times the
bundled studies never reach: MocoSumSquaredStateGoal, MocoControlGoal with
exponents 3 and 4, zero and all-zero weights, two goals of a kind, backward
differences, auxiliary derivatives behind accelerations, the lane and generic
back ends, grids past one stride of k_reduce_obj and one block of
k_integrand, t0 != 0, a tracking reference narrower than [t0, tf] with grid
times on its breaks, and every shard's own partial.

Every bound is eps T of the reference: T the sum of K_g A_g, A_g the running
absolute-value bound of goal g's share, K_g twice the roundings counted on
the device code's longest path (_objective_ref.roundings and the comments in
evaluate).  No entry is skipped.  The unmarked tests prove the reference
against closed forms and run the CPU oracle through the same matrix at the
same bounds; the gpu tests run the device."""
import copy
import json
import os

import numpy as np
import pytest

import _objective_ref as oref
from _objective_ref import EPS, LD
from mocohip import configs
from mocohip.problem import (ImplicitAuxiliaryDerivativesTerm, MocoControlGoal, MocoFinalTimeGoal,
                             MocoStateTrackingGoal, MocoSumSquaredStateGoal)
from mocohip.solver import HipNLP, OracleNLP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FDS = ("forward", "backward", "central")


# ---- the goal sets ----------------------------------------------------------

def _names(st):
    rep = st.problem.create_rep()
    return rep.state_names, rep.control_names


def mixed_goals(st, extra=()):
    """Control goals with exponents 2 (one weight 0, one 2.5), 3 and 4, a
    sum-squared-state goal (one weight 0, one 3), a final-time goal, a control
    goal whose weights are all 0 (no terms), then ``extra``."""
    s, c = _names(st)
    w2 = {c[0]: 0.0, c[-1]: 2.5} if len(c) > 1 else {c[0]: 2.5}
    return [MocoControlGoal("effort2", 1.5, 2, w2),
            MocoControlGoal("effort3", 0.7, 3),
            MocoControlGoal("effort4", 1e-3, 4),
            MocoSumSquaredStateGoal("states", 0.3, {s[0]: 0.0, s[1]: 3.0}),
            MocoFinalTimeGoal("final_time", 0.25),
            MocoControlGoal("dropped", 2.0, 2, {n: 0.0 for n in c}),
            *extra]


def _pendulum(N, scheme, tracking=False):
    st = configs.double_pendulum(N, scheme=scheme)
    extra = []
    if tracking:
        tab = configs.double_pendulum_swing_states()
        st.problem.model.add_table(tab)
        extra = [MocoStateTrackingGoal("tracking", 0.8, tab, {tab_name(tab, 1): 0.0})]
    st.problem.goals = mixed_goals(st, extra)
    return st


def tab_name(tab, i):
    return list(tab.columns)[i]


def _pendulum_tracking():
    """The double-pendulum effort study tracking the swing states (a table
    over [0, 2], breaks every 0.05), one state weight 0."""
    st = configs.double_pendulum_effort(4)
    tab = configs.double_pendulum_swing_states()
    st.problem.model.add_table(tab)
    st.problem.goals = [MocoStateTrackingGoal("tracking", 1.0, tab, {tab_name(tab, 2): 0.0}),
                        MocoControlGoal("effort", 0.001)]
    return st


def _sliding_mass():
    st = configs.sliding_mass(2)
    st.problem.goals = mixed_goals(st)
    return st


def _gait():
    st = configs.gait10dof18musc(2)
    track = next(g for g in st.problem.goals if isinstance(g, MocoStateTrackingGoal))
    st.problem.goals = mixed_goals(st, [track])
    return st


def _gait_aux():
    st = configs.gait10dof18musc(2, tendon_compliance=True, tendon_dynamics="implicit", dynamics="implicit")
    st.problem.goals = st.problem.goals + [ImplicitAuxiliaryDerivativesTerm("aux", 0.01)]
    return st


def _rajagopal80():
    st = configs.rajagopal80(2)
    st.problem.goals = [MocoControlGoal("effort3", 0.7, 3), MocoSumSquaredStateGoal("states", 0.3)]
    return st


def _no_goals():
    st = configs.double_pendulum(2)
    st.problem.goals = []
    return st


# name: (study, iterate kind, (t0, tf), schemes, back ends)
CASES = {}
for _N in (1, 63, 255, 256):    # G = 2, 64, 256, 257: k_integrand's block edge, k_reduce_obj's stride
    CASES[f"pendulum_trap_{_N}"] = (lambda N=_N: _pendulum(N, "trapezoidal"), "random", (0.13, 1.9), FDS, ("auto",))
for _N in (1, 32, 128, 256):    # G = 3, 65, 257, 513
    CASES[f"pendulum_hs_{_N}"] = (lambda N=_N: _pendulum(N, "hermite-simpson"), "random", (0.13, 1.9), FDS,
                                  ("auto",))
CASES.update({
    "sliding_mass": (_sliding_mass, "random", (0.13, 1.9), FDS, ("auto",)),
    "tracking_inside": (_pendulum_tracking, "random", (0.13, 1.9), FDS, ("auto",)),
    # N = 4 over [-0.5, 2.5]: mesh times -0.5, 0.25, 1, 1.75, 2.5 -- both ends
    # extrapolate, the inner three fall on breaks of the table
    "tracking_wider_on_breaks": (_pendulum_tracking, "random", (-0.5, 2.5), FDS, ("auto",)),
    "gait": (_gait, "physiological", (0.13, 1.9), FDS, ("auto", "lane", "generic")),
    "gait_aux_derivatives": (_gait_aux, "physiological", (0.13, 1.9), FDS, ("auto",)),
    "coupled_multipliers": (lambda: configs.double_pendulum_coupled(2, dynamics="implicit"), "random",
                            (0.13, 1.9), FDS, ("auto",)),
    "swingup_marker_final": (lambda: configs.double_pendulum_swingup(3), "random", (0.13, 1.9), FDS, ("auto",)),
    # forward only: the other two schemes add nothing new at this size; generic: the large size class
    "rajagopal80": (_rajagopal80, "physiological", (0.13, 1.9), ("forward",), ("auto", "generic")),
    "no_goals": (_no_goals, "random", (0.13, 1.9), FDS, ("auto",)),
})
MATRIX = [(c, fd) for c, v in CASES.items() for fd in v[3]]
DEVICE_MATRIX = [(c, fd, b) for c, v in CASES.items() for fd in v[3] for b in v[4]]


def _iterate(lay, kind, times):
    """Random within bounds (muscle models: the physiological iterate), t0 /
    tf as given; controls of both signs, one exactly 0."""
    if kind == "physiological":
        from test_gpu_parity import physiological_iterate
        x = physiological_iterate(lay, 0)
    else:
        x = lay.random_iterate(np.random.default_rng(7).uniform(-1, 1, lay.n))
    x[0], x[1] = times
    G, NS, NC = lay.G, lay.NS, lay.NC
    U = x[2 + NS * G:2 + (NS + NC) * G].reshape(G, NC)
    U[0, NC - 1], U[G - 1, 0] = -abs(U[0, NC - 1]), abs(U[G - 1, 0])
    U[G // 2, NC - 1] = 0.0
    assert (U < 0).any() and (U > 0).any() and (U == 0).any()
    return x


_CACHE = {}


def _case(name, fd):
    """(study, rep, options, x, reference), built once per (case, scheme)."""
    key = (name, fd)
    if key not in _CACHE:
        build, kind, times, _, _ = CASES[name]
        st = build()
        st.solver.optim_finite_difference_scheme = fd
        rep = st.problem.create_rep()
        opts = st.solver.options()
        lay = oref.Layout(rep, opts)
        src = OracleNLP(rep, opts)      # random_iterate is the library's (bit-equal on both)
        assert (src.n, src.G, src.NS, src.NC) == (lay.n, lay.G, lay.NS, lay.NC)
        x = _iterate(src, kind, times)
        src.close()
        goals = oref.resolve_goals(st, rep, lay)
        res = oref.evaluate(lay, goals, x)
        assert np.isfinite(float(res.f)) and np.all(np.isfinite(res.grad.astype(float)))
        _CACHE[key] = (st, rep, opts, x, lay, goals, res)
    return _CACHE[key]


def _backend_nlp(rep, opts, backend):
    saved = os.environ.pop("MOCOHIP_BACKEND", None)
    if backend != "auto":
        os.environ["MOCOHIP_BACKEND"] = backend
    try:
        return HipNLP(rep, opts)
    finally:
        os.environ.pop("MOCOHIP_BACKEND", None)
        if saved is not None:
            os.environ["MOCOHIP_BACKEND"] = saved


def _compare(label, nlp, x, res, partial=False):
    """eval_f, objective_terms (the device), eval_grad_f, the structural
    zeros and a second call, against the reference."""
    f = nlp.eval_f_partial(x) if partial else nlp.eval_f(x)
    gf = nlp.eval_grad_f_partial(x) if partial else nlp.eval_grad_f(x)
    terms = nlp.objective_terms(x) if hasattr(nlp, "objective_terms") and not partial else None
    r = oref.ratios(res, f, terms, gf)
    per_goal = ""
    if terms is not None and len(terms):
        assert len(terms) == len(res.terms)
        e = np.abs(terms.astype(LD) - res.terms)
        per_goal = " terms " + " ".join(
            f"{k}:{float(e[i] / (EPS * res.A_terms[i])) if res.A_terms[i] > 0 else float(e[i] > 0):.2f}"
            f"/K={res.K_terms[i]:.0f}" for i, k in enumerate(res.kinds))
    Kf = float(res.T_f / res.A_f) if res.A_f > 0 else 0.0
    Kg = float(np.max(np.where(res.A_grad > 0, res.T_grad / np.where(res.A_grad > 0, res.A_grad, 1), 0),
                      initial=0.0))
    print(f"[objective-ref] {label}: max err/(eps A): f {r['f'][0]:.2f} (K {Kf:.0f}) "
          f"grad {r['grad'][0]:.2f} (K <= {Kg:.0f}){per_goal}")
    f2 = nlp.eval_f_partial(x) if partial else nlp.eval_f(x)
    gf2 = nlp.eval_grad_f_partial(x) if partial else nlp.eval_grad_f(x)
    assert np.array_equal(np.array([f2]).view(np.uint64), np.array([f]).view(np.uint64))
    assert np.array_equal(gf2.view(np.uint64), gf.view(np.uint64))
    assert np.all(gf[res.zero] == 0.0), np.flatnonzero(gf[res.zero] != 0.0)
    assert np.all(res.grad[res.zero] == 0)
    if not res.kinds:
        assert f == 0.0 and np.all(gf == 0.0)
    assert r["f"][1], r
    if terms is not None:
        assert r["terms"][1], r
    assert r["grad"][1], r
    return f, gf


# ---- the reference against closed forms (CPU) --------------------------------

def _single_control_goal(fd, exponent=2):
    st = configs.sliding_mass(1)
    st.solver.transcription_scheme = "trapezoidal"
    st.solver.optim_finite_difference_scheme = fd
    st.problem.goals = [MocoControlGoal("effort", 1.5, exponent, {"/actuator": 2.5})]
    rep = st.problem.create_rep()
    lay = oref.Layout(rep, st.solver.options())
    return st, rep, lay


@pytest.mark.parametrize("fd", FDS)
def test_reference_quotient_of_a_square_is_the_closed_form(fd):
    """L = w v^2: the forward quotient is w (2 v + h), the backward one
    w (2 v - h), the central one 2 w v, with h the step fl(v +- h) really
    takes; the scalings W (tf - t0) quad_k around it."""
    st, rep, lay = _single_control_goal(fd)
    x = np.array([0.13, 1.9, 0.3, -0.2, 0.1, 0.4, -3.7, 1.3])   # 2 points: states, then controls
    assert lay.n == x.size and lay.G == 2
    res = oref.evaluate(lay, oref.resolve_goals(st, rep, lay), x)
    h, W, w, dur = LD(1e-8), LD(1.5), LD(2.5), LD(1.9) - LD(0.13)
    for k, col in enumerate((6, 7)):
        v = LD(x[col])
        hp, hm = LD(x[col] + 1e-8) - v, v - LD(x[col] - 1e-8)
        want = {"forward": w * hp * (2 * v + hp) / h, "backward": w * hm * (2 * v - hm) / h,
                "central": w * (hp + hm) * (2 * v + hp - hm) / (2 * h)}[fd]
        near = {"forward": w * (2 * v + h), "backward": w * (2 * v - h), "central": 2 * w * v}[fd]
        got = res.grad[col]
        # the long-double quotient cancels too: its own error is 2^-11 of the double bound eps A
        assert abs(got - W * dur * LD(0.5) * want) <= 8 * float(np.finfo(LD).eps) * res.A_grad[col]
        assert abs(got - W * dur * LD(0.5) * near) <= 4 * EPS * abs(v) / 1e-8 * abs(W * dur * w)
    f = W * dur * LD(0.5) * w * (LD(x[6]) ** 2 + LD(x[7]) ** 2)
    assert abs(res.f - f) <= 1e-17 * abs(f)
    assert abs(res.grad[1] - f / dur) <= 1e-17 * abs(f) and abs(res.grad[0] + f / dur) <= 1e-17 * abs(f)
    assert np.all(res.grad[2:6] == 0) and np.all(res.zero[2:6]) and not res.zero[[0, 1, 6, 7]].any()


def test_reference_odd_exponent_at_a_negative_control():
    """|v|^3 at v = -2: 8, and a quotient near d|v|^3/dv = -3 v^2 = -12."""
    st, rep, lay = _single_control_goal("central", 3)
    goal = oref.resolve_goals(st, rep, lay)[0]
    P = np.array([[0.0, 0.0, -2.0]])
    L, A = oref.integrand(goal, P, np.zeros(1), np.zeros(1, LD))
    assert L[0] == LD(2.5) * 8 and A[0] == L[0]
    x = np.array([0.0, 1.0, 0, 0, 0, 0, -2.0, -2.0])
    res = oref.evaluate(lay, [goal], x)
    assert abs(res.grad[6] - LD(1.5) * LD(0.5) * LD(2.5) * -12) <= 1e-6
    signed = copy.deepcopy(goal)
    signed.signed = True
    assert oref.integrand(signed, P, np.zeros(1), np.zeros(1, LD))[0][0] == -L[0]


def test_reference_tracking_term_at_a_break_and_extrapolated():
    st = _pendulum_tracking()
    rep = st.problem.create_rep()
    lay = oref.Layout(rep, st.solver.options())
    goal = oref.resolve_goals(st, rep, lay)[0]
    tab = goal.table
    assert tab.br[0] == 0.0 and tab.br[-1] == 2.0 and tab.br[5] == 0.25
    t = np.array([0.25, -0.5, 2.5, 0.0, 2.0])
    assert list(tab.segment(t)) == [5, 0, tab.nseg - 1, 0, tab.nseg - 1]
    v, a, d = tab.eval(goal.cols, t)

    def poly(s, dt):
        return sum(tab.cf[s][:, k] * LD(dt) ** k for k in range(tab.degree + 1))
    assert np.all(v[0] == tab.cf[5][:, 0])                     # at the break: the new segment's constant
    assert np.max(np.abs(v[0] - poly(4, tab.br[5] - tab.br[4]))) <= 1e-9   # and the spline is continuous there
    assert np.max(np.abs(v[1] - poly(0, -0.5))) <= 1e-17 * float(np.max(a[1]))
    assert np.max(np.abs(v[2] - poly(tab.nseg - 1, 2.5 - tab.br[-2]))) <= 1e-17 * float(np.max(a[2]))
    assert np.all(a >= np.abs(v))
    # the derivative: against a difference of the polynomial itself
    e = 1e-6
    assert np.max(np.abs(d[1] - (poly(0, -0.5 + e) - poly(0, -0.5 - e)) / (2 * e))) <= 1e-6 * float(np.max(a[1]))
    # the term: w (s - r)^2 with the zero weight kept as a term
    P = np.zeros((5, lay.NI))
    P[:, :lay.NS] = 0.3
    L, A = oref.integrand(goal, P, t, np.ones(5, LD))
    w = goal.w.astype(LD)
    assert (w == 0).sum() == 1
    assert np.max(np.abs(L - (w * (LD(0.3) - v) ** 2).sum(1))) <= 1e-17 * float(A.max())
    assert np.all(A >= L)


def test_reference_gives_the_sum_squared_state_integrands_of_the_reference_test():
    with open(os.path.join(GOLDEN, "sum_squared_state_integrands.json")) as fh:
        gold = json.load(fh)
    for case in gold["cases"]:
        st = configs.double_pendulum(1)
        weights = {f"/jointset/j{q[1]}/{q}/value": w for q, w in case["state_weights"].items()}
        st.problem.goals = [MocoSumSquaredStateGoal("states", 1.0, weights)]
        rep = st.problem.create_rep()
        lay = oref.Layout(rep, st.solver.options())
        goal = oref.resolve_goals(st, rep, lay)[0]
        P = np.zeros((1, lay.NI))
        for q, v in gold["coordinate_values"].items():
            P[0, rep.state_names.index(f"/jointset/j{q[1]}/{q}/value")] = v
        L, _ = oref.integrand(goal, P, np.zeros(1), np.zeros(1, LD))
        assert float(L[0]) == case["integrand"]
        # and the device's lowering holds the same terms
        ref = OracleNLP(rep, st.solver.options())
        x = np.zeros(ref.n)
        x[1] = 1.0
        x[2:2 + ref.NS * ref.G] = np.tile(P[0, :ref.NS], ref.G)
        assert ref.eval_f(x) == pytest.approx(case["integrand"], rel=1e-15)


# ---- the refusals (CPU) ------------------------------------------------------

def _refusals():
    out = []
    st = configs.double_pendulum(2)
    st.problem.goals = [MocoControlGoal("effort", 1.0, 2, {"/tau2": 3.0})]
    out.append((st, "Unrecognized control '/tau2'."))
    st = configs.double_pendulum(2)
    st.problem.goals = [MocoSumSquaredStateGoal("states", 1.0, {"/jointset/j0/q0/valu": 3.0})]
    out.append((st, "Weight provided with name '/jointset/j0/q0/valu' but this is not a recognized state."))
    st = _pendulum_tracking()
    st.problem.goals[0].state_weights = {"/jointset/j2/q2/value": 3.0}
    out.append((st, "Weight provided with name '/jointset/j2/q2/value' but this is not a recognized state."))
    return out


def test_unknown_weight_names_are_refused_like_the_reference():
    """MocoControlGoal.cpp:64-71, MocoSumSquaredStateGoal.cpp:37-45,
    MocoStateTrackingGoal.cpp:45-52: a weight for a control / state the model
    does not have throws."""
    import re
    for st, msg in _refusals():
        with pytest.raises(ValueError, match=re.escape(msg)):
            st.problem.create_rep()


# ---- the oracle against the reference (CPU) ----------------------------------

@pytest.mark.parametrize("name,fd", MATRIX)
def test_oracle_against_reference(name, fd):
    st, rep, opts, x, lay, goals, res = _case(name, fd)
    ref = OracleNLP(rep, opts)
    _compare(f"oracle {name} {fd}", ref, x, res)
    ref.close()


SHARDS = ((0, 2), (2, 3), (3, 5))


def _shard_study(fd):
    st = _pendulum(5, "hermite-simpson")
    st.solver.optim_finite_difference_scheme = fd
    rep = st.problem.create_rep()
    lay = oref.Layout(rep, st.solver.options())
    full = OracleNLP(rep, st.solver.options())
    x = _iterate(full, "random", (0.13, 1.9))
    full.close()
    return st, rep, lay, x, oref.resolve_goals(st, rep, lay)


def _check_shards(label, make, fd):
    st, rep, lay, x, goals = _shard_study(fd)
    whole = oref.evaluate(lay, goals, x)
    fs, gs = LD(0), np.zeros(lay.n, LD)
    for a, b in SHARDS:
        res = oref.evaluate(lay, goals, x, intervals=(a, b))
        assert (res.terms[res.kinds.index("final_time")] != 0) == (b == 5)   # endpoint terms: last shard only
        sh = make(rep, st.solver.options(a, b))
        _compare(f"{label} shard [{a},{b}) {fd}", sh, x, res, partial=True)
        sh.close()
        fs, gs = fs + res.f, gs + res.grad
    assert abs(fs - whole.f) <= 1e-17 * whole.A_f and np.all(np.abs(gs - whole.grad) <= 1e-17 * whole.A_grad)


@pytest.mark.parametrize("fd", FDS)
def test_oracle_shard_partials_against_reference(fd):
    _check_shards("oracle", OracleNLP, fd)


def _mutations(goals):
    """Four ways the objective could be subtly wrong, applied to the reference."""
    kinds = [g.kind for g in goals]
    ssq, trk = kinds.index("sum_squared_state"), kinds.index("state_tracking")
    cube = next(i for i, g in enumerate(goals) if g.kind == "control" and g.exponent == 3)
    out = {}
    m = copy.deepcopy(goals); m[ssq].w[0] *= 1 + 1e-4; out["one weight times 1 + 1e-4"] = m
    m = copy.deepcopy(goals); m[ssq].idx[[0, 1]] = m[ssq].idx[[1, 0]]; out["two term indices swapped"] = m
    assert goals[ssq].w[0] != goals[ssq].w[1]
    m = copy.deepcopy(goals); m[cube].signed = True; out["|v|^3 as v^3"] = m
    m = copy.deepcopy(goals); m[trk].cols = (m[trk].cols + 1) % len(m[trk].cols); out["tracked column shifted"] = m
    return out


def _check_sensitivity(label, make):
    st = _pendulum(32, "hermite-simpson", tracking=True)
    rep = st.problem.create_rep()
    opts = st.solver.options()
    lay = oref.Layout(rep, opts)
    nlp = make(rep, opts)
    x = _iterate(nlp, "random", (0.13, 1.9))
    goals = oref.resolve_goals(st, rep, lay)
    f, gf = _compare(f"{label} sensitivity base", nlp, x, oref.evaluate(lay, goals, x))
    nlp.close()
    for what, mutated in _mutations(goals).items():
        res = oref.evaluate(lay, mutated, x)
        vf = float(abs(LD(f) - res.f) / (EPS * res.T_f))
        e, T = np.abs(gf.astype(LD) - res.grad), EPS * res.T_grad
        vg = float(np.max(np.where(T > 0, e / np.where(T > 0, T, 1), np.where(e > 0, np.inf, 0))))
        print(f"[objective-ref] {label} mutation '{what}': violation factor f {vf:.3g} grad {vg:.3g}")
        assert max(vf, vg) > 1.0, what


def test_bounds_reject_mutations_of_the_reference_oracle():
    _check_sensitivity("oracle", OracleNLP)


# ---- the device against the reference (GPU) ----------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,fd,backend", DEVICE_MATRIX)
def test_device_against_reference(name, fd, backend):
    st, rep, opts, x, lay, goals, res = _case(name, fd)
    gpu = _backend_nlp(rep, opts, backend)
    want = {"auto": "", "lane": "generated-lane:", "generic": "generic"}[backend]
    assert gpu.backend()[0].startswith(want), gpu.backend()
    assert gpu.n == lay.n
    _compare(f"device {name} {fd} {backend} [{gpu.backend()[0]}]", gpu, x, res)
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fd", FDS)
def test_device_shard_partials_against_reference(fd):
    _check_shards("device", HipNLP, fd)


@pytest.mark.gpu
def test_bounds_reject_mutations_of_the_reference_device():
    _check_sensitivity("device", HipNLP)


# ---- the four lane-goal families on one problem (GPU) -------------------------

def _four_family_study(fd, kinds):
    """The coupled double pendulum with a muscle (test_muscle_outputs'
    _coupled_muscle_study: Hermite-Simpson, N = 2, implicit dynamics, so that
    the input has coordinates, speeds, a muscle state, a control, acceleration
    variables, multipliers at every grid point and slacks at the midpoints)
    with one goal of each kind in ``kinds`` in front of its effort goal, in the
    families' launch order: joint reaction (14), acceleration tracking (15),
    muscle output (17), metabolics (18)."""
    from mocohip.problem import MocoJointReactionGoal, MocoOutputGoal
    from test_acceleration_tracking import _with_goal
    from test_metabolics import _with_metabolics
    from test_muscle_outputs import _coupled_muscle_study
    st = _coupled_muscle_study("implicit", False)
    st.solver.optim_finite_difference_scheme = fd
    base = list(st.problem.goals)
    st.problem.goals = []
    if 14 in kinds:
        st.problem.add_goal(MocoJointReactionGoal("reaction", 0.5, joint_path="j1", loads_frame="child"))
    if 15 in kinds:
        sw = configs.double_pendulum_swing_states()
        _with_goal(st, "accel", 0.75, ["/bodyset/b1", "/bodyset/b0"], sw.times,
                   {"q0": sw.columns["/jointset/j0/q0/value"], "q1": sw.columns["/jointset/j1/q1/value"]})
    if 17 in kinds:
        st.problem.add_goal(MocoOutputGoal("output", 1.5, output_path="/forceset/flexor|tendon_force"))
    if 18 in kinds:
        _with_metabolics(st, "/forceset/flexor")   # (inserts its goal "met" in front)
        st.problem.goals.append(st.problem.goals.pop(0))
    st.problem.goals += base
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("fd", FDS)
def test_four_lane_goal_families_together(fd):
    """One goal of each of kinds 14, 15, 17 and 18 on one problem, whose
    directions go down every branch of grad_entry (t0 / tf, states, controls,
    acceleration variables, multipliers) and whose slacks have no lane.  Each
    goal's objective term has the bits it has in the study holding that goal
    alone; grad f equals the gradient without the four plus the four separate
    contributions within the bound of test_acceleration_tracking's
    test_two_goals_and_kinds_12_14_15_together (8 eps on the summands'
    magnitudes plus 1e-12 |grad|); every family's contribution is non-zero
    somewhere; the slack entries, and every entry no family moves on its own,
    carry the bits of the study without the four."""
    kinds = (14, 15, 17, 18)
    names = {14: "reaction", 15: "accel", 17: "output", 18: "met"}
    runs, x = {}, None
    for key in (kinds, *((k,) for k in kinds), ()):
        st = _four_family_study(fd, key)
        nlp = HipNLP(st.problem.create_rep(), st.solver.options())
        if x is None:
            G, NS = nlp.G, nlp.NS
            r = np.random.default_rng(12)
            x = nlp.random_iterate(r.uniform(-1, 1, nlp.n))
            x[0], x[1] = 0.1, 0.9
            x[2:2 + NS * G].reshape(G, NS)[:, 4:] = r.uniform(0.2, 0.8, (G, NS - 4))   # activations
            N = nlp.opts.num_mesh_intervals
            XM = 2 + (NS + nlp.NC) * G
            XL = XM + nlp.NM * G
            DB = XL + nlp.NSL * N
            assert nlp.NM * G > 0 and nlp.NSL * N > 0 and nlp.NDV * G > 0 and DB + nlp.NDV * G == nlp.n
        assert nlp.n == len(x)
        goal_names = [g.name for g in st.problem.goals]
        runs[key] = (dict(zip(goal_names, nlp.objective_terms(x))), nlp.eval_grad_f(x))
        nlp.close()
    terms, g_all = runs[kinds]
    g_0 = runs[()][1]
    assert list(terms)[:4] == [names[k] for k in kinds]
    for k in kinds:
        alone = runs[(k,)][0][names[k]]
        assert alone != 0.0 and np.float64(terms[names[k]]).tobytes() == np.float64(alone).tobytes(), (k, fd)
    parts = [runs[(k,)][1] - g_0 for k in kinds]
    want, mag = g_0.copy(), np.abs(g_0)
    for p in parts:
        want = want + p
        mag = mag + np.abs(p)
    assert (np.abs(g_all - want) <= 8 * EPS * mag + 1e-12 * np.abs(g_all)).all()
    for p in parts:
        assert np.abs(p).max() > 0
    still = np.ones(len(x), bool)
    for k in kinds:
        still &= runs[(k,)][1].view(np.uint64) == g_0.view(np.uint64)
    assert still[XL:DB].all()   # the slacks: no lane in any family
    assert g_all[still].tobytes() == g_0[still].tobytes()
    # t0, tf, states or controls, and the acceleration variables do move; no goal reads the multipliers,
    # whose entries hold the multiplier term's non-zero values, so a stray write there would show
    assert not still[[0, 1]].any() and not still[2:XM].all() and not still[DB:].all()
    assert (g_0[XM:XL] != 0.0).all()
