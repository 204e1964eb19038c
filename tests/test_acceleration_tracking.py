"""MocoAccelerationTrackingGoal on the dynamics-stage lanes (include/mocohip.h
MH_GOAL_ACCELERATION_TRACKING; k_accel_tracking, k_lane_goal_grad,
mh_eval_frame_accelerations).

The checker is a NumPy restatement built on test_joint_reaction.body_motion
(every body's pose, spatial velocity V and spatial acceleration A in ground
about the ground origin, zero base acceleration, accumulated along
test_frame_distance.forward_kinematics' motion list): the acceleration of a
point at r is a0 + alpha x r + omega x (v + omega x r).  It uses no library code
under test.  Its own accuracy is shown first against closed forms (1e-12
relative) and against a difference stencil of mocohip.model's positions along a
smooth motion; the project's 1e-10 (|want| + 1) is then the device's margin.

udot of the explicit contexts: test_joint_reaction.solved_udot (the
restatement's own forward dynamics) on the muscle-free models, the CPU oracle's
DAE on gait10dof18musc."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.model import DataTable
from mocohip.problem import (FrameReference, MocoAccelerationTrackingGoal, MocoAngularVelocityTrackingGoal,
                             MocoJointReactionGoal)
from mocohip.tape import write_tape
from test_frame_tracking import _info
from test_joint_reaction import _grad_index, _rel, body_motion, solved_udot
from test_marker_tracking import quadrature, table_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_BUILD = os.path.join(ROOT, "opensim-moco_amd", "csrc", "build", "mh_build")
EPS = np.finfo(float).eps
AT = MocoAccelerationTrackingGoal
SUFFIXES = ("acceleration_x", "acceleration_y", "acceleration_z")


# ---- the restatement --------------------------------------------------------

def resolve_frame(model, path):
    """(body name or "ground", location in it) of a frame path, resolved here."""
    if path in ("/ground", "ground"):
        return "ground", np.zeros(3)
    off = next((f for f in model.offset_frames.values() if path in (f.path, f.name)), None)
    if off is not None:
        return off.body, np.asarray(off.translation, float)
    return path.replace("/bodyset/", ""), np.zeros(3)


def frame_acceleration(model, path, q, u, ud):
    """The linear acceleration in ground of the origin of the frame at path."""
    body, loc = resolve_frame(model, path)
    if body == "ground":
        return np.zeros(3)
    R, p, V, A = body_motion(model, np.asarray(q, float), np.asarray(u, float), np.asarray(ud, float))[0][body]
    r = p + R @ loc
    w, v, al, a0 = V[:3], V[3:], A[:3], A[3:]
    return a0 + np.cross(al, r) + np.cross(w, v + np.cross(w, r))


def goal_frames(goal):
    """[(path, weight)] of a goal, in the goal's order."""
    return [(p, float(goal.frame_weights.get(p, 1.0))) for p in (goal.frame_paths or goal.reference.labels)]


def reference_at(ms, goal, t):
    """[frames, 3]: the goal's reference at t from the compiled table."""
    name = goal.reference_name()
    ti, cols = ms.compiled.table_index[name], ms.compiled.table_columns[name]
    return np.array([[table_value(ms.struct.model, ti, cols.index(f"{p}/{s}"), t)[0] for s in SUFFIXES]
                     for p, _ in goal_frames(goal)])


def integrand(model, ms, goal, q, u, ud, t):
    ref = reference_at(ms, goal, t)
    return sum(w * float(np.sum((frame_acceleration(model, p, q, u, ud) - ref[i]) ** 2))
               for i, (p, w) in enumerate(goal_frames(goal)))


# ---- CPU: the restatement itself ----------------------------------------------

def test_restatement_against_closed_forms():
    """1e-12 relative: a pendulum point at radius r, r (udot t - u^2 r_hat);
    the double pendulum's second link; a slider, a = udot dir; a ground frame,
    a = 0; an offset frame on a body spinning at a constant rate, the
    omega x (omega x r) term alone."""
    m = configs.n_link_pendulum(1)
    m.add_offset_frame("tip", "b0", (0.4, 0.3, 0.25))
    for q, u, ud in ((0.3, -1.7, 2.9), (-2.2, 4.1, -0.6), (1.4, 0.0, 0.7)):
        c, s = math.cos(q), math.sin(q)
        rh, th = np.array([c, s, 0.0]), np.array([-s, c, 0.0])
        a = frame_acceleration(m, "/bodyset/b0", [q], [u], [ud])
        assert _rel(a, 1.0 * (ud * th - u * u * rh)) <= 1e-12
        r = np.array([c * 1.4 - s * 0.3, s * 1.4 + c * 0.3, 0.0])   # the tip, in the plane
        a = frame_acceleration(m, "/bodyset/b0/tip", [q], [u], [ud])
        assert _rel(a, ud * np.cross([0, 0, 1.0], r) - u * u * r) <= 1e-12
        assert np.array_equal(frame_acceleration(m, "/ground", [q], [u], [ud]), np.zeros(3))
        # constant rate: omega x (omega x r) with the tip's full position (its z does not enter)
        om, rf = np.array([0.0, 0.0, u]), r + np.array([0.0, 0.0, 0.25])
        a = frame_acceleration(m, "b0/tip" if False else "/bodyset/b0/tip", [q], [u], [0.0])
        assert np.abs(a - np.cross(om, np.cross(om, rf))).max() <= 1e-12 * (np.abs(a).max() + 1e-300) or u == 0.0
    m2 = configs.n_link_pendulum(2)
    for q, u, ud in (((0.3, -0.8), (-1.7, 2.2), (2.9, -3.1)), ((-2.2, 1.9), (4.1, 0.4), (-0.6, 5.0))):
        a0, a1 = q[0], q[0] + q[1]
        w0, w1, d0, d1 = u[0], u[0] + u[1], ud[0], ud[0] + ud[1]
        want = (d0 * np.array([-math.sin(a0), math.cos(a0), 0]) - w0 * w0 * np.array([math.cos(a0), math.sin(a0), 0])
                + d1 * np.array([-math.sin(a1), math.cos(a1), 0]) - w1 * w1 * np.array([math.cos(a1), math.sin(a1), 0]))
        assert _rel(frame_acceleration(m2, "/bodyset/b1", q, u, ud), want) <= 1e-12
    sm = configs.sliding_mass(2).problem.model
    body = next(iter(sm.bodies))
    for q, u, ud in ((0.7, -1.2, 3.3), (-4.0, 2.0, -0.25)):
        assert _rel(frame_acceleration(sm, "/bodyset/" + body, [q], [u], [ud]), np.array([ud, 0.0, 0.0])) <= 1e-12


def _gimbal_qt(t):
    t = np.asarray(t, float)
    q = configs.gimbal_motion(t)
    u = configs.gimbal_motion_rates(t)
    a = {"qx": -2.4 * np.sin(2.0 * t + 0.3), "qy": -6.3 * np.cos(3.0 * t), "qz": 0.0 * t}
    return q, u, a


def _knee_qt(t):
    t = np.asarray(t, float)
    q, u = configs.spline_knee_motion(t)
    a = {"hip": -4.5 * np.sin(3.0 * t), "knee": -3.2 * np.cos(2.0 * t + 0.4)}
    return q, u, a


@pytest.mark.parametrize("name", ["gimbal", "spline_knee"])
def test_restatement_against_the_second_time_derivative_of_position(name):
    """mocohip.model's frame_pose_in_ground along a smooth q(t), u = dq/dt,
    udot = d2q/dt2: the gimbal (three rotation axes in one body: the crm(V, s)
    terms) and spline_knee_model (spline rotation and translation: d2 u^2).
    Fourth-order central second difference at step h,
      f'' = (-f(-2h) + 16 f(-h) - 30 f(0) + 16 f(h) - f(2h)) / (12 h^2),
    truncation error h^4 / 90 |f^(6)| and rounding error (the coefficients sum
    to 64 in magnitude) 64 e |f| / (12 h^2) with e = 8 eps the relative error
    allowed to a computed position.  |f^(6)| is estimated from the same
    positions by a sixth central difference at step 0.02 over the sample times,
    and doubled.  h = 2e-3: truncation about 1e-8, rounding about 4e-9, on
    accelerations of order 10.  spline_knee: the sample times keep the knee's
    whole stencil (and the estimate's) inside one piece of its splines, where
    the position is smooth."""
    if name == "gimbal":
        m = configs.gimbal_frame_tracking(2).problem.model
        paths, qt, times = ["/bodyset/body", "/bodyset/body/sensor"], _gimbal_qt, np.linspace(0.05, 0.45, 9)
    else:
        m = configs.spline_knee_model(slider_foot=False)
        paths, qt = ["/bodyset/thigh", "/bodyset/shank", "/bodyset/shank/imu"], _knee_qt
        knots = np.array([-2.0, -1.6, -1.2, -0.8, -0.4, 0.0, 0.2])
        times = []
        for t in np.linspace(0.02, 0.58, 57):
            kn = qt(np.array([t - 0.06, t, t + 0.06]))[0]["knee"]
            if np.searchsorted(knots, kn.min()) == np.searchsorted(knots, kn.max()):
                times.append(t)
        times = np.array(times[::4])
        assert len(times) >= 5
    names = [c.name for c in m.coordinates()]
    h = 2e-3

    def pos(path, t):
        q = qt(np.array([t]))[0]
        return m.frame_pose_in_ground(path, {n: float(q[n][0]) for n in names})[0]
    worst = 0.0
    for path in paths:
        for t in times:
            f = [pos(path, t + k * h) for k in (-2, -1, 0, 1, 2)]
            want = (-f[0] + 16.0 * f[1] - 30.0 * f[2] + 16.0 * f[3] - f[4]) / (12.0 * h * h)
            e = 0.02
            g = [pos(path, t + k * e) for k in (-3, -2, -1, 0, 1, 2, 3)]
            f6 = np.abs(g[0] - 6 * g[1] + 15 * g[2] - 20 * g[3] + 15 * g[4] - 6 * g[5] + g[6]).max() / e ** 6
            tol = h ** 4 / 90.0 * 2.0 * f6 + 64.0 * 8 * EPS * (np.abs(f[2]).max() + 1.0) / (12.0 * h * h)
            q, u, a = qt(np.array([t]))
            got = frame_acceleration(m, path, [q[n][0] for n in names], [u[n][0] for n in names],
                                     [a[n][0] for n in names])
            worst = max(worst, float(np.abs(got - want).max() / tol))
            assert np.abs(got - want).max() <= tol, (path, t, got, want, tol)
            assert tol <= 1e-6 * (np.abs(want).max() + 1.0)   # the check has teeth
    print(f"{name}: worst |restated - second difference| / tol = {worst:.3e}")


# ---- the studies --------------------------------------------------------------

def _with_goal(st, name, weight, paths, times, coords, frame_weights=None, dynamics=None):
    """Adds to st a MocoAccelerationTrackingGoal whose reference is the second
    time difference of the frames' positions along the coordinate columns
    (data to track; nothing is checked against it)."""
    m = st.problem.model
    ref = configs.accelerations_from_coordinates(m, paths, times, coords)
    g = AT(name, weight, reference=ref, frame_weights=frame_weights or {}, table_name=name + "_ref")
    m.add_table(g.reference_table(m))
    st.problem.add_goal(g)
    if dynamics:
        st.solver.multibody_dynamics_mode = dynamics
    return st


def _pendulum(n, scheme, dynamics, second=False):
    """The reference's pendulum study at n intervals: its goal "tracking" on b0
    and b1, and (second) a second goal on a rotated offset frame of b1 (weight
    0.5) and on ground."""
    def make(goal=True, weight=None):
        st = configs.double_pendulum_acceleration_tracking(None, n, scheme, "central", dynamics)
        st.problem.model.add_offset_frame("tip", "b1", (0.3, -0.2, 0.1), (0.2, 0.5, -0.4))
        if not goal:
            st.problem.goals = [g for g in st.problem.goals if not isinstance(g, AT)]
            return st
        if weight is not None:
            st.problem.goals[-1].weight = weight
        if second:
            sw = configs.double_pendulum_swing_states()
            _with_goal(st, "second", 0.25, ["/bodyset/b1/tip", "/ground"], sw.times,
                       {"q0": sw.columns["/jointset/j0/q0/value"], "q1": sw.columns["/jointset/j1/q1/value"]},
                       {"/bodyset/b1/tip": 0.5})
        return st
    return make


def _gimbal(goal=True, weight=None):
    st = configs.gimbal_frame_tracking(2)
    st.solver.multibody_dynamics_mode = "implicit"
    if goal:
        t = np.linspace(0.0, 0.5, 26)
        _with_goal(st, "accel", 0.5 if weight is None else weight, ["/bodyset/body/sensor", "/bodyset/body"], t,
                   configs.gimbal_motion(t), {"/bodyset/body/sensor": 2.0})
    return st


def _spline_knee(dynamics):
    def make(goal=True, weight=None):
        st = configs.spline_knee(2, slider_foot=True)
        st.solver.multibody_dynamics_mode = dynamics
        if goal:
            t = np.linspace(0.0, 0.6, 31)
            q = dict(configs.spline_knee_motion(t)[0], slide=0.05 * np.sin(4.0 * t))
            _with_goal(st, "accel", 1.5 if weight is None else weight, ["/bodyset/shank/imu", "/bodyset/thigh"], t, q,
                       {"/bodyset/thigh": 0.25})
        return st
    return make


def _coupled(goal=True, weight=None):
    st = configs.double_pendulum_coupled(2, dynamics="explicit")
    if goal:
        sw = configs.double_pendulum_swing_states()
        _with_goal(st, "accel", 0.75 if weight is None else weight, ["/bodyset/b1", "/bodyset/b0"], sw.times,
                   {"q0": sw.columns["/jointset/j0/q0/value"], "q1": sw.columns["/jointset/j1/q1/value"]})
    return st


def _gait(goal=True, weight=None):
    if goal:
        st = configs.gait10dof18musc_accel_track_few(3)
        if weight is not None:
            next(g for g in st.problem.goals if isinstance(g, AT)).weight = weight
        return st
    st = configs.gait10dof18musc(3)
    st.problem.model.add_offset_frame("imu_torso", "torso", (-0.05, 0.3, 0.02), (0.2, -0.1, 0.4))
    return st


# case -> (study builder, "generic" to force the interpreter for g and J, muscle-free?)
CASES = {
    "pendulum_hs_2_explicit": (_pendulum(2, "hermite-simpson", "explicit"), "", True),
    "pendulum_hs_3_implicit": (_pendulum(3, "hermite-simpson", "implicit", second=True), "", True),
    "pendulum_trap_3_explicit": (_pendulum(3, "trapezoidal", "explicit", second=True), "", True),
    "pendulum_trap_2_implicit": (_pendulum(2, "trapezoidal", "implicit"), "", True),
    "gimbal_2_implicit": (_gimbal, "", True),
    "spline_knee_2_explicit": (_spline_knee("explicit"), "", True),
    "spline_knee_2_implicit": (_spline_knee("implicit"), "", True),
    "coupled_2_explicit": (_coupled, "", True),
    "gait_3_generic": (_gait, "generic", False),
    "gait_3_generated": (_gait, "", False),
}
MATRIX = [(c, fd) for c in CASES for fd in (("central", "forward", "backward") if c.startswith("pendulum")
                                            else ("forward",) if c.startswith("gait") else ("central",))]


def _study(case, fd, goal=True, weight=None):
    st = CASES[case][0](goal)
    if weight is not None:   # every acceleration-tracking goal of the study
        for g in st.problem.goals:
            if isinstance(g, AT):
                g.weight = weight
    st.solver.optim_finite_difference_scheme = fd
    return st


def _nlp(case, st, interval=None):
    from mocohip.solver import HipNLP
    generic = CASES[case][1] == "generic"
    if generic:
        os.environ["MOCOHIP_BACKEND"] = "generic"
    try:
        nlp = HipNLP(st.problem.create_rep(), st.solver.options(*(interval or ())))
    finally:
        os.environ.pop("MOCOHIP_BACKEND", None)
    if case.startswith("gait"):
        assert nlp.backend()[0].startswith("generic" if generic else "generated:"), nlp.backend()
    return nlp


def _iterate(case, nlp, st):
    """A random iterate (implicit mode: random accelerations too).  spline_knee:
    the knee well inside a spline piece.  gait: the muscle model's working
    range.  Times inside the references' rows."""
    x = nlp.random_iterate(np.random.default_rng(27).uniform(-1, 1, nlp.n))
    G, NS, NC = nlp.G, nlp.NS, nlp.NC
    r = np.random.default_rng(28)
    if case.startswith("gait"):
        x[2:2 + NS * G] = r.uniform(0.05, 0.5, NS * G)
        x[2 + NS * G:2 + (NS + NC) * G] = r.uniform(0.05, 0.4, NC * G)
        x[0], x[1] = 0.3, 1.2
        return x
    x[0], x[1] = 0.05, 0.45
    S = x[2:2 + NS * G].reshape(G, NS)
    nq = nlp.NQ
    S[:, :nq] = r.uniform(-1.0, 1.0, (G, nq))
    S[:, nq:2 * nq] = r.uniform(-2.0, 2.0, (G, nq))
    if case.startswith("spline"):
        names = [c.name for c in st.problem.model.coordinates()]
        S[:, names.index("knee")] = -1.8 + 0.4 * r.integers(0, 4, G) + r.uniform(-0.1, 0.1, G)
        S[:, names.index("slide")] = r.uniform(-0.05, 0.05, G)
    return x


def _udot(b, rows, ts):
    """udot at rows of point inputs: the rows' own (implicit), the
    restatement's forward dynamics (muscle-free), the CPU oracle's DAE (gait)."""
    NS, NC, NDV, nq = b["NS"], b["NC"], b["NDV"], b["NQ"]
    rows = np.atleast_2d(rows)
    if b["implicit"]:
        return rows[:, NS + NC:NS + NC + nq]
    if b["free"]:
        return np.array([solved_udot(b["model"], b["ms"], r[:nq], r[nq:2 * nq], r[NS:NS + NC],
                                     r[NS + NC + NDV:NS + NC + NDV + b["NM"]], t) for r, t in zip(rows, ts)])
    return b["oracle"].eval_dae(np.column_stack([ts, rows]))[:, :nq]


def _restated_L(b, rows, ts):
    """[rows, goals]: every goal's integrand by the restatement."""
    rows = np.atleast_2d(rows)
    ud = _udot(b, rows, ts)
    nq = b["NQ"]
    return np.array([[integrand(b["model"], b["ms"], g, r[:nq], r[nq:2 * nq], a, t) for g, _ in b["goals"]]
                     for r, a, t in zip(rows, ud, ts)])


@functools.lru_cache(maxsize=None)
def _base(case):
    """Per case, once: the iterate, the layout, the device's accelerations of
    every goal's frames at every grid point, the restated integrands."""
    st = _study(case, "forward")
    nlp = _nlp(case, st)
    d = {"st": st, "model": st.problem.model, "ms": nlp.rep, "free": CASES[case][2]}
    d["grid"], d["quad"] = quadrature(nlp)
    x = d["x"] = _iterate(case, nlp, st)
    for k in ("G", "NS", "NC", "NDV", "NM", "NSL", "NI", "NQ", "n"):
        d[k] = getattr(nlp, k)
    d["implicit"] = bool(nlp.implicit)
    d["idx"] = np.array([[_grad_index(nlp, k, j) for j in range(nlp.NI - nlp.NSL)] for k in range(nlp.G)])
    d["P"] = nlp.point_inputs(x)
    d["t"] = x[0] + (x[1] - x[0]) * d["grid"]
    d["goals"] = [(g, gi) for gi, g in enumerate(st.problem.goals) if isinstance(g, AT)]
    d["acc"] = {g.name: nlp.frame_accelerations(x, g.name) for g, _ in d["goals"]}
    d["dae"] = nlp.eval_dae(np.column_stack([d["t"], d["P"]]))
    nlp.close()
    if not d["free"]:
        from mocohip.solver import OracleNLP
        st0 = _study(case, "forward", False)   # the same DAE; the oracle does not know the goal
        d["oracle"] = OracleNLP(st0.problem.create_rep(), st0.solver.options(), threads=8)
        assert d["oracle"].NI == d["NI"]
    d["L"] = _restated_L(d, d["P"], d["t"])   # [G, goals]
    return d


@functools.lru_cache(maxsize=None)
def _evaluated(case, fd):
    """Everything the GPU tests of one (case, scheme) read, computed once: with
    the goals f, the terms, grad f (twice); the same study without them; with
    them at weight 0."""
    b = _base(case)
    x = b["x"]
    st = _study(case, fd)
    nlp = _nlp(case, st)
    d = {"st": st, "h": st.solver.fd_step if st.solver.fd_step > 0 else 1e-8}
    assert nlp.n == b["n"]
    stride = (2 if fd == "central" else 1) * (nlp.NI - nlp.NSL + 2) + 1
    assert (nlp.G * stride) % 64 != 0 and nlp.G % 64 != 0   # the tail guards run
    d["f"], d["terms"], d["grad"] = nlp.eval_f(x), nlp.objective_terms(x), nlp.eval_grad_f(x)
    d["f2"], d["grad2"] = nlp.eval_f(x), nlp.eval_grad_f(x)
    nlp.close()
    nlp0 = _nlp(case, _study(case, fd, False))
    assert nlp0.n == b["n"]
    d["f0"], d["grad0"], d["terms0"] = nlp0.eval_f(x), nlp0.eval_grad_f(x), nlp0.objective_terms(x)
    nlp0.close()
    nlpz = _nlp(case, _study(case, fd, True, 0.0))
    d["fz"], d["gradz"] = nlpz.eval_f(x), nlpz.eval_grad_f(x)
    nlpz.close()
    return d


# ---- CPU: lowering, builder, layout query -------------------------------------

def _terms(st, gi):
    rep = st.problem.create_rep()
    G = rep.struct.goals[gi]
    tb = G.term_begin
    return (G, list(rep._gidx[tb:tb + G.term_count]), list(rep._gcol[tb:tb + G.term_count]),
            np.array(rep._gw[tb:tb + G.term_count]), rep)


def test_lowering_terms_columns_weights_and_offset_frames():
    """Four terms per frame in kind 9's layout: zeros for a body frame, an
    offset frame's translation carried and its orientation ignored, ground as
    body -1, the table's columns, the weights; the frame_paths selection."""
    st = _pendulum(3, "hermite-simpson", "implicit", second=True)()
    gi = [i for i, g in enumerate(st.problem.goals) if isinstance(g, AT)]
    G, gidx, gcol, gw, rep = _terms(st, gi[0])
    bi = rep.compiled.body_index
    assert (G.kind, G.term_count, G.weight) == (abi.MH_GOAL_ACCELERATION_TRACKING, 8, 1.0) and G.kind == 15
    cols = rep.compiled.table_columns["tracking_reference"]
    assert G.table == rep.compiled.table_index["tracking_reference"]
    assert gidx == [bi["b0"]] * 4 + [bi["b1"]] * 4
    assert gcol == [cols.index(f"/bodyset/b0/{s}") for s in SUFFIXES] + [-1] + \
        [cols.index(f"/bodyset/b1/{s}") for s in SUFFIXES] + [-1]
    assert list(gw) == [0.0, 0.0, 0.0, 1.0] * 2
    G, gidx, gcol, gw, rep = _terms(st, gi[1])
    assert (G.kind, G.term_count, G.weight) == (15, 8, 0.25)
    assert gidx == [bi["b1"]] * 4 + [-1] * 4
    assert list(gw) == [0.3, -0.2, 0.1, 0.5, 0.0, 0.0, 0.0, 1.0]   # the tip's orientation (0.2, 0.5, -0.4) is not used
    # frame_paths selects columns of the reference, in its own order
    g = st.problem.goals[gi[1]]
    g.frame_paths = ["/ground"]
    G, gidx, gcol, gw, rep = _terms(st, gi[1])
    cols = rep.compiled.table_columns["second_ref"]
    assert G.term_count == 4 and gidx == [-1] * 4 and gcol[:3] == [cols.index(f"/ground/{s}") for s in SUFFIXES]


def _bad_goals():
    t = np.linspace(0.0, 2.0, 5)
    z = np.zeros((5, 1, 3))
    return [
        (AT("g", reference=FrameReference(t, ["/bodyset/b0"], z), frame_paths=["/bodyset/b1"]),
         "Expected frame_paths to match one of the column labels in the acceleration reference, but frame path "
         "'/bodyset/b1' not found in the reference labels.", True),
        (AT("g", reference=FrameReference(t, ["/bodyset/b0", "/bodyset/b0"], np.zeros((5, 2, 3)))),
         "appears more than once", False),
        (AT("g", reference=FrameReference(t, ["/bodyset/b9"], z)), "no frame '/bodyset/b9' in the model", False),
        (AT("g", reference=FrameReference(t, ["/bodyset/b0"], z), frame_weights={"/bodyset/b0": -1.0}),
         "negative weight -1", False),
    ]


def test_lowering_reports_the_reference_errors(tmp_path):
    """The reference's messages (MocoAccelerationTrackingGoal.cpp:56-63,
    checkRedundantLabels) and this project's, from problem.py and (where the
    description can carry the goal) from mh_build alike; a states reference,
    prescribed kinematics and MocoParameters are refused."""
    for goal, msg, python_only in _bad_goals():
        st = configs.double_pendulum_effort(2)
        m = st.problem.model
        with pytest.raises(ValueError) as e:
            m.add_table(goal.reference_table(m))
            st.problem.add_goal(goal)
            st.problem.create_rep()
        assert msg in str(e.value), (msg, str(e.value))
    # through mh_build: the goal's frame weights name a frame the table lacks / the model lacks / a negative weight
    for mutate, msg in ((lambda g: g.frame_weights.update({"/bodyset/b0": -1.0}), "negative weight -1"),):
        st = configs.double_pendulum_acceleration_tracking(None, 2)
        mutate(st.problem.goals[-1])
        desc = tmp_path / "bad.mhdesc"
        write_description(st, str(desc))
        r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "bad.tape")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (msg, r.stderr)
    with pytest.raises(ValueError, match="a states reference cannot be given"):
        AT("g", states_reference=configs.double_pendulum_swing_states(),
           frame_paths=["/bodyset/b0"]).tracked_frame_paths()
    with pytest.raises(ValueError, match="no reference"):
        AT("g").tracked_frame_paths()
    t = np.linspace(0.0, 1.0, 4)
    st = configs.gait10dof18musc_inverse(2)
    g = AT("g", reference=FrameReference(t, ["/bodyset/pelvis"], np.zeros((4, 1, 3))))
    st.problem.model.add_table(g.reference_table(st.problem.model))
    st.problem.add_goal(g)
    with pytest.raises(NotImplementedError, match="MocoAccelerationTrackingGoal with prescribed kinematics"):
        st.problem.create_rep()
    st = configs.oscillator_mass(2)
    body = next(iter(st.problem.model.bodies))
    g = AT("g", reference=FrameReference(t, ["/bodyset/" + body], np.zeros((4, 1, 3))))
    st.problem.model.add_table(g.reference_table(st.problem.model))
    st.problem.add_goal(g)
    with pytest.raises(NotImplementedError, match="MocoAccelerationTrackingGoal with MocoParameters"):
        st.problem.create_rep()
    desc = tmp_path / "par.mhdesc"
    write_description(st, str(desc))
    r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "par.tape")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "MocoAccelerationTrackingGoal with MocoParameters" in r.stderr, r.stderr


BUILDER_CASES = {
    "pendulum": lambda: configs.double_pendulum_acceleration_tracking(None, 2),
    "pendulum_implicit_trapezoidal": lambda: configs.double_pendulum_acceleration_tracking(
        None, 3, "trapezoidal", "forward", "implicit"),
    "pendulum_two_goals": _pendulum(3, "hermite-simpson", "implicit", second=True),
    "gimbal": _gimbal,
    "spline_knee": _spline_knee("explicit"),
    "coupled": _coupled,
    "gait_few": lambda: configs.gait10dof18musc_accel_track_few(3),
    "gait_implicit": lambda: configs.gait10dof18musc_accel_track(4, dynamics="implicit"),
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    problem.py; the description carries one goal acceleration_tracking record
    per goal."""
    st = BUILDER_CASES[name]()
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    n = sum(isinstance(g, AT) for g in st.problem.goals)
    assert n >= 1 and sum(ln.startswith("goal acceleration_tracking ") for ln in desc.read_text().splitlines()) == n
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


def _bad_problems():
    """(study builder, mutation of its mh_problem, message, error code).  In
    the pendulum study goal 1 is the acceleration-tracking goal."""
    pend = lambda: configs.double_pendulum_acceleration_tracking(None, 2)   # noqa: E731
    cols = np.zeros(64, np.int32)
    bounds = (abi.mh_bounds * 1)()
    targets = (abi.mh_parameter_target * 1)()

    def seti(field, k, v):
        def f(p):
            getattr(p, field)[p.goals[1].term_begin + k] = v
        return f

    def setg(**kw):
        def f(p):
            for k, v in kw.items():
                setattr(p.goals[1], k, v)
        return f

    def prescribe(p):
        p.prescribed_kinematics = 1
        p.kinematics_table = 0
        p.kinematics_column = abi.iptr(cols)

    def parameter(p):   # one parameter: the mass of body 0
        bounds[0].lower, bounds[0].upper = 0.5, 2.0
        targets[0].parameter, targets[0].kind, targets[0].index, targets[0].element = 0, abi.MH_PARAM_BODY_MASS, 0, 0
        p.nparameters, p.nparameter_targets = 1, 1
        p.parameter_bounds, p.parameter_targets = bounds, targets

    def presc_study():   # the tracking goal first
        st = configs.double_pendulum_acceleration_tracking(None, 2, dynamics="implicit")
        st.problem.goals = st.problem.goals[1:] + st.problem.goals[:1]
        return st

    def presc_first(p):   # (goal 0 is the tracking goal there)
        prescribe(p)

    I, U = abi.MH_ERR_INVALID, abi.MH_ERR_UNSUPPORTED
    return [
        (pend, setg(term_count=7), "acceleration tracking goal needs four terms per frame", I),
        (pend, setg(term_count=9), "acceleration tracking goal needs four terms per frame", I),
        (pend, setg(term_count=-4), "acceleration tracking goal needs four terms per frame", I),
        (pend, setg(table=-1), "bad table", I),
        (pend, setg(table=99), "bad table", I),
        (pend, seti("goal_index", 2, 1), "a frame's terms name different bodies", I),
        (pend, lambda p: [seti("goal_index", k, 2)(p) for k in range(4)], "index 2 out of range", I),
        (pend, lambda p: [seti("goal_index", k, -2)(p) for k in range(4)], "index -2 out of range", I),
        (pend, seti("goal_column", 1, -1), "column out of range", I),
        (pend, seti("goal_column", 6, 6), "column out of range", I),
        (pend, seti("goal_weight", 7, -0.5), "negative frame weight", I),
        (pend, seti("goal_weight", 3, math.nan), "negative frame weight", I),
        (pend, setg(kind=13), "unknown kind 13", I),
        (pend, setg(kind=16), "unknown kind 16", I),
        (presc_study, presc_first, "acceleration tracking goal with prescribed kinematics", U),
        (pend, parameter, "acceleration tracking goal with MocoParameters", U),
    ]


def test_layout_query_accepts_the_goal_and_refuses_what_create_refuses():
    """mh_get_nlp_info_for (host only): the goal changes no layout count;
    every refusal comes with its code and message; kinds 13 and 16 are unknown."""
    lib = abi.load_mocohip()
    for case in CASES:
        (rc, a, _), (rc0, b, _) = _info(CASES[case][0](True)), _info(CASES[case][0](False))
        assert rc == 0 and rc0 == 0, lib.mh_last_error().decode()
        assert (a.n, a.m, a.nnz_jac_g, a.num_grid_points, a.num_states, a.num_controls) == \
            (b.n, b.m, b.nnz_jac_g, b.num_grid_points, b.num_states, b.num_controls)
    for make, mutate, msg, code in _bad_problems():
        rc, _, _ = _info(make(), mutate)
        assert rc == code and msg in lib.mh_last_error().decode(), (msg, rc, lib.mh_last_error().decode())
        assert lib.mh_last_error().decode().startswith("goal ")   # the message names the goal


# ---- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_accelerations_against_the_restatement(case):
    """mh_eval_frame_accelerations at every grid point of the iterate against
    the restatement, per component within 1e-10 (|want| + 1).  Implicit: the
    iterate's (random) accelerations.  Explicit, muscle-free: the restatement's
    own solved udot.  gait10dof18musc: the CPU oracle's DAE udot.  The two gait
    cases (g and J on the interpreter / on the generated back end) give the
    same bits."""
    b = _base(case)
    nq = b["NQ"]
    ud = _udot(b, b["P"], b["t"])
    worst, big = 0.0, 0.0
    for g, _ in b["goals"]:
        got = b["acc"][g.name]
        assert got.shape == (b["G"], len(goal_frames(g)), 3)
        for k in range(b["G"]):
            for i, (p, _) in enumerate(goal_frames(g)):
                want = frame_acceleration(b["model"], p, b["P"][k][:nq], b["P"][k][nq:2 * nq], ud[k])
                err = np.abs(got[k, i] - want) / (np.abs(want) + 1.0)
                worst, big = max(worst, float(err.max())), max(big, float(np.abs(want).max()))
                assert (err <= 1e-10).all(), (case, g.name, k, p, got[k, i], want)
    assert big > 1e-2
    print(f"{case}: worst |a - restated| / (|restated| + 1) = {worst:.3e}")
    if case.startswith("gait"):
        other = _base("gait_3_generic" if case == "gait_3_generated" else "gait_3_generated")
        for name, v in b["acc"].items():
            assert np.array_equal(v, other["acc"][name])


@pytest.mark.gpu
@pytest.mark.parametrize("dyn", ["pendulum_hs_2", "spline_knee_2"])
def test_explicit_matches_implicit_fed_the_explicit_udot(dyn):
    """The explicit context's accelerations at its iterate equal, within 1e-10
    (|want| + 1), those of an implicit context of the same model whose
    acceleration inputs are the udot of the explicit context's mh_eval_dae."""
    b = _base(dyn + "_explicit")
    other = {"pendulum_hs_2": _pendulum(2, "hermite-simpson", "implicit"),
             "spline_knee_2": _spline_knee("implicit")}[dyn]
    from mocohip.solver import HipNLP
    st = other()
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    NS, NC, nq = b["NS"], b["NC"], b["NQ"]
    assert nlp.NS == NS and nlp.NC == NC and nlp.NDV >= nq and nlp.implicit
    rows = np.zeros((b["G"], 1 + nlp.NI))
    rows[:, 0] = b["t"]
    rows[:, 1:1 + NS + NC] = b["P"][:, :NS + NC]
    rows[:, 1 + NS + NC:1 + NS + NC + nq] = b["dae"][:, :nq]
    for gi, g in enumerate(st.problem.goals):
        if not isinstance(g, AT):
            continue
        got, want = b["acc"][g.name], nlp.eval_frame_accelerations(gi, rows)
        assert np.abs(want).max() > 1e-2
        assert (np.abs(got - want) <= 1e-10 * (np.abs(want) + 1.0)).all(), (g.name, got, want)
    nlp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_objective_against_the_restatement(case, fd):
    """Each goal's entry of mh_eval_objective_terms and f - f0: weight *
    duration * sum_k quad_k L_k of the restatement within 1e-10 (|want| + 1);
    the other goals' terms are those of the study without the goal, bit for
    bit; two evaluations give the same bits."""
    b, d = _base(case), _evaluated(case, fd)
    x = b["x"]
    total, gis = 0.0, []
    for j, (goal, gi) in enumerate(b["goals"]):
        want = goal.weight * (x[1] - x[0]) * float(b["quad"] @ b["L"][:, j])
        got = d["terms"][gi]
        print(f"{case} {fd} {goal.name}: term {got:.17g} restated {want:.17g} |diff| {abs(got - want):.3e}")
        assert abs(got - want) <= 1e-10 * (abs(want) + 1.0)
        assert want > 0.0
        total += want
        gis.append(gi)
    assert abs((d["f"] - d["f0"]) - total) <= 1e-10 * (abs(total) + 1.0) + 8 * EPS * abs(d["f0"])
    assert np.array_equal(np.delete(d["terms"], gis), d["terms0"]) and len(d["terms0"]) >= 1
    assert d["f"] == d["f2"] and np.array_equal(d["grad"], d["grad2"], equal_nan=True)
    assert np.isfinite(d["grad"]).all() and math.isfinite(d["f"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_gradient_against_the_restated_quotients(case, fd):
    """mh_eval_grad_f minus the gradient of the study without the goals, over
    every direction (t0, tf, states, controls, accelerations, multipliers),
    against k_grad's quotient formulas applied to the restated L at the
    perturbed inputs.  Tolerance in the form of test_joint_reaction's gradient
    test without its truncation term (both sides form the same quotient): per
    quotient 1e-8 |want| + 8 dv / h, dv the measured value error of the terms
    (<= 1e-10 relative) on |L| + 1 plus 64 eps (max |L| + 1); plus 64 eps
    |grad0|.  t0 / tf: -+ sum_k quad_k L_k plus the time quotients, whose lanes
    move the references' time (and, on gait, the ground-reaction loads')."""
    b, d = _base(case), _evaluated(case, fd)
    x, G, h = b["x"], b["G"], d["h"]
    dur, quad, g = x[1] - x[0], b["quad"], b["grid"]
    W = np.array([goal.weight for goal, _ in b["goals"]])
    L = b["L"] @ W                                                   # [G]
    diff = d["grad"] - d["grad0"]
    rel = max(abs(d["terms"][gi] - goal.weight * dur * float(quad @ b["L"][:, j]))
              / (abs(goal.weight * dur * float(quad @ b["L"][:, j])) + 1.0)
              for j, (goal, gi) in enumerate(b["goals"]))            # measured value error, <= 1e-10
    dv = rel * (np.abs(L) + 1.0) + 64 * EPS * (np.abs(L).max() + 1.0)
    nd = b["NI"] - b["NSL"]

    def quotients(lanes):
        """lanes(step) -> (rows [n, NI], times [n]); the scheme's quotient of W . L."""
        if fd == "central":
            return (_restated_L(b, *lanes(h)) @ W - _restated_L(b, *lanes(-h)) @ W) / (2.0 * h)
        if fd == "forward":
            return (_restated_L(b, *lanes(h)) @ W - np.repeat(L, len(lanes(h)[1]) // G)) / h
        return (np.repeat(L, len(lanes(h)[1]) // G) - _restated_L(b, *lanes(-h)) @ W) / h

    def input_lanes(step):
        rows = np.repeat(b["P"], nd, axis=0)
        for k in range(G):
            for s in range(nd):
                rows[k * nd + s, s] += step
        return rows, np.repeat(b["t"], nd)
    q = quotients(input_lanes).reshape(G, nd)
    worst = 0.0
    for k in range(G):
        for s in range(nd):
            scale = dur * quad[k]
            want = scale * q[k, s]
            i = b["idx"][k, s]
            tol = scale * (1e-8 * abs(q[k, s]) + 8 * dv[k] / h) + 64 * EPS * abs(d["grad0"][i])
            worst = max(worst, abs(diff[i] - want) / tol)
            assert abs(diff[i] - want) <= tol, (k, s, diff[i], want, tol)
    acc = float(quad @ L)
    for c in (0, 1):
        seed = (1.0 - g) if c == 0 else g
        qt = quotients(lambda step: (b["P"], b["t"] + step * seed))
        want = (-acc if c == 0 else acc) + dur * float(quad @ qt)
        tol = 1e-10 * (abs(acc) + 1.0) + dur * float(quad @ (1e-8 * np.abs(qt) + 8 * dv / h)) \
            + 64 * EPS * abs(d["grad0"][c])
        worst = max(worst, abs(diff[c] - want) / tol)
        assert abs(diff[c] - want) <= tol, (c, diff[c], want, tol)
    print(f"{case} {fd}: worst |grad f - ref| / tol = {worst:.3e}")


def _chain_inputs(b):
    """The point inputs an implicit context's integrand depends on: value,
    speed and acceleration variable of every coordinate on a tracked chain."""
    model, nq = b["model"], b["NQ"]
    qidx = model.coordinate_index()
    parent = {j.child: j for j in model.joints}
    on = set()
    for goal, _ in b["goals"]:
        for p, _ in goal_frames(goal):
            body = resolve_frame(model, p)[0]
            while body != "ground":
                j = parent[body]
                on.update(qidx[ax.func.coord] for ax in j.axes if ax.func.kind != abi.MH_FN_CONSTANT)
                body = j.parent
    na = b["NS"] + b["NC"]
    return sorted(on), sorted([s for s in on] + [nq + s for s in on] + [na + s for s in on])


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_exact_zeros_and_nothing_else_moves(case, fd):
    """Implicit dynamics: every entry outside t0, tf and the tracked chains'
    q, u and udot keeps the bits of the same study without the goal, and those
    entries do move.  Explicit: every state, control and multiplier entry may
    move; the slacks keep their bits.  In both: the goal at weight 0 changes
    nothing anywhere, f included."""
    b, d = _base(case), _evaluated(case, fd)
    moved = d["grad"] != d["grad0"]
    touched = np.zeros(b["n"], bool)
    touched[[0, 1]] = True
    if b["implicit"]:
        on, inputs = _chain_inputs(b)
        assert len(on) >= 1
        touched[b["idx"][:, inputs].ravel()] = True
        assert moved[b["idx"][:, inputs]].all() and moved[0] and moved[1]
        if case.startswith("spline"):   # the foot's slider is off every tracked chain
            assert len(on) < b["NQ"]
    else:
        touched[b["idx"].ravel()] = True
        assert moved[b["idx"][:, :2 * b["NQ"]]].all() and moved[0] and moved[1]
    assert np.array_equal(d["grad"][~touched], d["grad0"][~touched], equal_nan=True)
    assert (~touched).sum() > 0 or not b["implicit"]
    assert d["fz"] == d["f0"] and np.array_equal(d["gradz"], d["grad0"], equal_nan=True)


def _contributions(make_parts, fd, x_from):
    """grad f of a study with all of the goals, and of the studies with the
    base goals plus each one alone."""
    from mocohip.solver import HipNLP
    out = []
    for st in make_parts:
        st.solver.optim_finite_difference_scheme = fd
        nlp = HipNLP(st.problem.create_rep(), st.solver.options())
        out.append((nlp.eval_f(x_from), nlp.eval_grad_f(x_from)))
        nlp.close()
    return out


@pytest.mark.gpu
def test_two_goals_and_kinds_12_14_15_together():
    """Two kind-15 goals on one problem, and kinds 12 + 14 + 15 on one: the
    gradient equals the gradient without them plus the separate contributions,
    within the bound of test_joint_reaction's shard-sum test (8 eps on the
    summands' magnitudes plus 1e-12 |grad|)."""
    case = "pendulum_hs_3_implicit"
    b = _base(case)
    x = b["x"]

    def only(names):
        st = _study(case, "central")
        st.problem.goals = [g for g in st.problem.goals if not isinstance(g, AT) or g.name in names]
        return st
    (f_all, g_all), (f_a, g_a), (f_b, g_b), (f_0, g_0) = _contributions(
        [only({"tracking", "second"}), only({"tracking"}), only({"second"}), only(set())], "central", x)
    want = g_0 + (g_a - g_0) + (g_b - g_0)
    bound = 8 * EPS * (np.abs(g_0) + np.abs(g_a - g_0) + np.abs(g_b - g_0)) + 1e-12 * np.abs(g_all)
    assert (np.abs(g_all - want) <= bound).all()
    assert np.abs(g_a - g_0).max() > 0 and np.abs(g_b - g_0).max() > 0
    assert abs(f_all - (f_0 + (f_a - f_0) + (f_b - f_0))) <= 8 * EPS * (abs(f_0) + abs(f_a) + abs(f_b))

    def mixed(kinds):
        st = configs.spline_knee(2, slider_foot=True)   # kind 12 and the effort goal
        st.solver.multibody_dynamics_mode = "explicit"
        if 12 not in kinds:
            st.problem.goals = [g for g in st.problem.goals if not isinstance(g, MocoAngularVelocityTrackingGoal)]
        if 14 in kinds:
            st.problem.add_goal(MocoJointReactionGoal("knee_reaction", 0.5, joint_path="knee", loads_frame="child"))
        if 15 in kinds:
            t = np.linspace(0.0, 0.6, 31)
            q = dict(configs.spline_knee_motion(t)[0], slide=0.05 * np.sin(4.0 * t))
            _with_goal(st, "accel", 1.5, ["/bodyset/shank/imu", "/bodyset/foot"], t, q)
        return st
    bk = _base("spline_knee_2_explicit")
    parts = _contributions([mixed({12, 14, 15}), mixed({12}), mixed({14}), mixed({15}), mixed(set())], "central",
                           bk["x"])
    (f_all, g_all), (_, g12), (_, g14), (_, g15), (_, g_0) = parts
    want = g_0 + (g12 - g_0) + (g14 - g_0) + (g15 - g_0)
    bound = 8 * EPS * (np.abs(g_0) + np.abs(g12 - g_0) + np.abs(g14 - g_0) + np.abs(g15 - g_0)) \
        + 1e-12 * np.abs(g_all)
    assert (np.abs(g_all - want) <= bound).all()
    for gk in (g12, g14, g15):
        assert np.abs(gk - g_0).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pendulum_hs_3_implicit", "pendulum_trap_3_explicit", "gait_3_generated"])
def test_shards_sum_to_the_whole(case):
    """mh_eval_f_partial / mh_eval_grad_f_partial over 2 shards, with the
    bounds of test_joint_reaction's shard test."""
    fd = "forward" if case.startswith("gait") else "central"
    b, d = _base(case), _evaluated(case, fd)
    x, G = b["x"], b["G"]
    st = _study(case, fd)
    N = st.solver.num_mesh_intervals
    step = (G - 1) // N
    cut = 1
    parts = []
    for lo, hi in ((0, cut), (cut, N)):
        sh = _nlp(case, st, (lo, hi))
        parts.append((sh.eval_f_partial(x), sh.eval_grad_f_partial(x)))
        sh.close()
    fsum = parts[0][0] + parts[1][0]
    assert abs(fsum - d["f"]) <= 8 * EPS * (abs(parts[0][0]) + abs(parts[1][0]))
    assert parts[0][0] != 0.0 and parts[1][0] != 0.0
    kcut = cut * step
    for k in range(G):
        for i in b["idx"][k]:
            if k < kcut:
                assert parts[0][1][i] == d["grad"][i] and parts[1][1][i] == 0.0, (k, i)
            elif k > kcut:
                assert parts[1][1][i] == d["grad"][i] and parts[0][1][i] == 0.0, (k, i)
    gsum = parts[0][1] + parts[1][1]
    bound = 8 * EPS * (np.abs(parts[0][1]) + np.abs(parts[1][1])) + 1e-12 * np.abs(d["grad"])
    assert (np.abs(gsum - d["grad"]) <= bound).all()


@pytest.mark.gpu
def test_refusals_and_the_entry_s_own():
    """mh_create refuses what the layout query refuses, before device work;
    mh_eval_frame_accelerations refuses a goal that is not of kind 15 and a
    call with no rows."""
    from mocohip.solver import HipNLP
    for make, mutate, msg, _ in _bad_problems():
        st = make()
        rep = st.problem.create_rep()
        mutate(rep.struct)
        with pytest.raises(RuntimeError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            HipNLP(rep, st.solver.options())
    st = configs.double_pendulum_acceleration_tracking(None, 2)
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    rows = np.zeros((1, 1 + nlp.NI))
    for goal in (0, -1, 2, 99):
        with pytest.raises(RuntimeError, match="is not an acceleration tracking goal"):
            nlp.eval_frame_accelerations(goal, rows)
    with pytest.raises(ValueError, match="no goal 'nothing'"):
        nlp.frame_accelerations(np.zeros(nlp.n), "nothing")
    assert nlp.eval_frame_accelerations(1, rows).shape == (1, 2, 3)
    with pytest.raises(RuntimeError, match="0 rows"):   # np = 0 is refused
        nlp.eval_frame_accelerations(1, np.zeros((0, 1 + nlp.NI)))
    nlp.close()


@pytest.mark.gpu
def test_reference_double_pendulum_acceleration_tracking():
    """testMocoGoals.cpp:327-361 at N = 20: solve double_pendulum_effort
    (explicit), read b0's and b1's accelerations from the solution
    (frame_accelerations, the reference's analyze(...|linear_acceleration)),
    solve again with effort weight 0.001 plus the tracking goal: states and
    controls match the effort solution within the reference's 1e-1.  Then once
    more with implicit dynamics."""
    effort_study = configs.double_pendulum_effort(20)
    effort = effort_study.solve()
    assert effort.metadata["success"] == "true", effort.metadata
    probe = configs.double_pendulum_acceleration_tracking(None, 20)
    nlp = probe.create_nlp()
    acc = nlp.frame_accelerations(effort, "tracking")
    nlp.close()
    assert acc.shape == (len(effort.time), 2, 3) and np.abs(acc).max() > 0.1
    ref = FrameReference(np.asarray(effort.time, float), ["/bodyset/b0", "/bodyset/b1"], acc)
    for dynamics in ("explicit", "implicit"):
        sol = configs.double_pendulum_acceleration_tracking(ref, 20, dynamics=dynamics).solve()
        ds = float(np.abs(sol.states - effort.states).max())
        dc = float(np.abs(sol.controls - effort.controls).max())
        print(f"{dynamics}: {sol.metadata['num_iterations']} iterations, status {sol.metadata.get('status')}, "
              f"objective {sol.metadata['objective']}, max |states - effort| {ds:.3e}, max |controls - effort| "
              f"{dc:.3e}")
        assert sol.metadata["success"] == "true", sol.metadata
        assert np.allclose(sol.time, effort.time)
        assert ds <= 1e-1 and dc <= 1e-1
