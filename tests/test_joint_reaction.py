"""MocoJointReactionGoal on the dynamics stage of the generic interpreter
(include/mocohip.h MH_GOAL_JOINT_REACTION; k_joint_reaction,
k_lane_goal_grad, mh_eval_joint_reaction).

The checker is a NumPy Newton-Euler and momentum restatement built on
tests/test_frame_distance.forward_kinematics: from (t, q, u, udot) every body's
spatial velocity and acceleration along its motion list, then per body the rate
of change of its linear momentum and of its angular momentum about the ground
origin; the load a joint applies to its child is the sum of those over the
child's subtree minus the subtree's weight and external loads, shifted to the
joint frame's origin and expressed as the header states.  It never uses
mocohip.model kinematics or library code under test.  Its own accuracy is shown
first against closed forms (1e-12 relative); the project's 1e-10 (|want| + 1)
is then the device's margin.

Muscles are not restated: on gait10dof18musc the checks are the whole-body
momentum balance at the pelvis (the muscle forces must cancel), the mobility
forces at the pins, the exact zeros, determinism and the shard sums; the
gradient is checked against the restatement on the muscle-free shapes."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.model import body_fixed_xyz
from mocohip.model import DataTable
from mocohip.problem import MocoJointReactionGoal
from mocohip.splines import SimmSpline
from mocohip.tape import write_tape
from test_frame_distance import forward_kinematics
from test_frame_tracking import _diff6, _info
from test_marker_tracking import quadrature, table_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_BUILD = os.path.join(ROOT, "opensim-moco_amd", "csrc", "build", "mh_build")
EPS = np.finfo(float).eps
JR = MocoJointReactionGoal
MEASURES = ("moment-x", "moment-y", "moment-z", "force-x", "force-y", "force-z")


# ---- the restatement --------------------------------------------------------

def _d2(f, q, qidx):
    """Second derivative of a coordinate function."""
    if f.kind == abi.MH_FN_SIMMSPLINE:
        return f.scale * SimmSpline(f.x, f.y)(q[qidx[f.coord]], 2)
    return 0.0


def _crm(V, S):
    """Spatial motion cross product V x S, both (angular, linear at the ground origin)."""
    return np.concatenate([np.cross(V[:3], S[:3]), np.cross(V[:3], S[3:]) + np.cross(V[3:], S[:3])])


def body_motion(model, q, u, ud):
    """body -> (R, p, V, A): pose, spatial velocity and spatial acceleration
    in ground about the ground origin, accumulated along the entries that the
    body's joint adds to forward_kinematics' motion list; and the list."""
    qidx = model.coordinate_index()
    pose = forward_kinematics(model, np.asarray(q, float))
    out = {"ground": (np.eye(3), np.zeros(3), np.zeros(6), np.zeros(6))}
    for j in model.tree_order():
        own = pose[j.child][2][len(pose[j.parent][2]):]
        driven = [ax for ty in (abi.MH_AXIS_TRANSLATION, abi.MH_AXIS_ROTATION) for ax in j.axes
                  if ax.type == ty and ax.func.kind != abi.MH_FN_CONSTANT]
        assert len(driven) == len(own)
        V, A = out[j.parent][2].copy(), out[j.parent][3].copy()
        for (s, dv, rot, a, pivot), ax in zip(own, driven):
            S = np.concatenate([a, np.cross(pivot, a)]) if rot else np.concatenate([np.zeros(3), a])
            thd = dv * u[s]
            thdd = dv * ud[s] + _d2(ax.func, q, qidx) * u[s] * u[s]
            A = A + S * thdd + _crm(V, S) * thd
            V = V + S * thd
        out[j.child] = (pose[j.child][0], pose[j.child][1], V, A)
    return out, pose


def momentum_rates(model, ms, q, u, ud, t, gravity=True, external=True):
    """body -> the 6-vector (moment about the ground origin, force) that must
    act on the body alone: d/dt of its angular and linear momentum minus its
    weight and its external loads (ExternalForce tables at time t)."""
    mot, pose = body_motion(model, q, u, ud)
    g = np.asarray(model.gravity, float) if gravity else np.zeros(3)
    out = {}
    for name, B in model.bodies.items():
        R, p, V, A = mot[name]
        w, vO, al, aO = V[:3], V[3:], A[:3], A[3:]
        c = p + R @ np.asarray(B.com, float)
        vc = vO + np.cross(w, c)
        ac = aO + np.cross(al, c) + np.cross(w, vc)
        ixx, iyy, izz, ixy, ixz, iyz = (float(v) for v in B.inertia)
        Ig = R @ np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]]) @ R.T
        dp = B.mass * ac
        dh = np.cross(c, dp) + Ig @ al + np.cross(w, Ig @ w)
        f = dp - B.mass * g
        n = dh - np.cross(c, B.mass * g)
        out[name] = np.concatenate([n, f])
    if external:
        for e in model.external_forces:   # ms: the problem rep (compiled tables)
            ti, cols = ms.compiled.table_index[e.table], ms.compiled.table_columns[e.table]

            def vec(ident):
                return np.array([table_value(ms.struct.model, ti, cols.index(ident + sfx), t)[0]
                                 for sfx in ("x", "y", "z")])
            F, P, T = vec(e.force_identifier), vec(e.point_identifier), vec(e.torque_identifier)
            out[e.body] = out[e.body] - np.concatenate([np.cross(P, F) + T, F])
    return out, mot, pose


def subtree_load(model, rates, body):
    """The sum of the rates over the body and its descendants."""
    kids = {}
    for j in model.joints:
        kids.setdefault(j.parent, []).append(j.child)
    total, stack = np.zeros(6), [body]
    while stack:
        b = stack.pop()
        total = total + rates[b]
        stack.extend(kids.get(b, []))
    return total


def resolve(model, goal):
    """(joint, child?, expressed-in body, R_EO, six weights, denominator) of a goal, resolved here."""
    joint = next(j for j in model.joints if goal.joint_path in (j.name, "/jointset/" + j.name))
    child = goal.loads_frame == "child"
    path = goal.expressed_in_frame_path
    if path:
        off = next((f for f in model.offset_frames.values() if path in (f.path, f.name)), None)
        if off is not None:
            e, R = off.body, body_fixed_xyz(off.orientation)
        else:
            e, R = ("ground" if path in ("/ground", "ground") else path.replace("/bodyset/", "")), np.eye(3)
    else:
        e = joint.child if child else joint.parent
        R = body_fixed_xyz(joint.orient_in_child if child else joint.orient_in_parent)
    chosen = list(goal.reaction_measures) or list(MEASURES)
    w = np.array([float(goal.reaction_weights.get(m, 1.0)) if m in chosen else 0.0 for m in MEASURES])
    den = sum(float(b.mass) for b in model.bodies.values())
    gm = float(np.linalg.norm(model.gravity))
    if gm > EPS ** 0.875:
        den *= gm
    return joint, child, e, R, w, den


def reaction(model, ms, goal, q, u, ud, t):
    """(r [6], L): the goal's load and integrand at (t, q, u, udot)."""
    joint, child, e, R_EO, w, den = resolve(model, goal)
    rates, mot, _ = momentum_rates(model, ms, q, u, ud, t)
    F = subtree_load(model, rates, joint.child)
    n, f = F[:3], F[3:]
    if child:
        Rb, pb = mot[joint.child][0], mot[joint.child][1]
        o = pb + Rb @ np.asarray(joint.loc_in_child, float)
        mom, frc = n - np.cross(o, f), f
    else:
        Rp, pp = mot[joint.parent][0], mot[joint.parent][1]
        o = pp + Rp @ np.asarray(joint.loc_in_parent, float)
        mom, frc = -(n - np.cross(o, f)), -f
    RGE = mot[e][0] @ R_EO
    r = np.concatenate([RGE.T @ mom, RGE.T @ frc])
    return r, float(w @ (r * r)) / den


def generalized_forces(model, ms, q, u, ud, t, gravity=True, external=True):
    """Inverse dynamics by the restatement: tau_s = sum over the motion-list
    entries of coordinate s of (d value / d q) S . (the load on the entry's body)."""
    rates, mot, pose = momentum_rates(model, ms, q, u, ud, t, gravity, external)
    tau = np.zeros(len(q))
    for j in model.tree_order():
        F = subtree_load(model, rates, j.child)
        for s, dv, rot, a, pivot in pose[j.child][2][len(pose[j.parent][2]):]:
            S = np.concatenate([a, np.cross(pivot, a)]) if rot else np.concatenate([np.zeros(3), a])
            tau[s] += dv * float(S @ F)
    return tau


def applied_mobility_forces(model, q, u, controls, mult):
    """Coordinate actuators, springs and the couplers' -G^T lambda."""
    qidx = model.coordinate_index()
    tau = np.zeros(len(q))
    for i, a in enumerate(model.actuators):
        assert not hasattr(a, "points")
        tau[qidx[a.coordinate]] += controls[i] * a.optimal_force
    for sp in model.springs:
        s = qidx[sp.coordinate]
        tau[s] += -sp.stiffness * (q[s] - sp.rest_length) - sp.viscosity * u[s]
    for i, k in enumerate(model.constraints):
        f, ci = k.function, qidx[k.function.coord]
        d1 = f.scale * (SimmSpline(f.x, f.y)(q[ci], 1) if f.kind == abi.MH_FN_SIMMSPLINE else f.a)
        tau[ci] -= k.scale_factor * d1 * mult[i]
        tau[qidx[k.dependent]] += mult[i]
    return tau


def solved_udot(model, ms, q, u, controls, mult, t):
    """Forward dynamics by the restatement: M udot = applied - bias."""
    nq = len(q)
    bias = generalized_forces(model, ms, q, u, np.zeros(nq), t)
    M = np.array([generalized_forces(model, ms, q, np.zeros(nq), np.eye(nq)[i], t, False, False)
                  for i in range(nq)]).T
    return np.linalg.solve(M, applied_mobility_forces(model, q, u, controls, mult) - bias)


# ---- the studies ------------------------------------------------------------

def _pendulum(n, scheme, dynamics):
    return lambda reaction=True: configs.double_pendulum_joint_reaction(n, scheme, "central", dynamics, reaction)


def _gimbal(reaction=True):
    """gimbal_frame_tracking's model (a three-axis joint with offset joint
    frames) and goals, with the gimbal's loads on the child in the rotated
    sensor frame and on the parent in the parent joint frame."""
    st = configs.gimbal_frame_tracking(2)
    if reaction:
        st.problem.add_goal(JR("gimbal_child", 0.5, joint_path="gimbal", loads_frame="child",
                               expressed_in_frame_path="/bodyset/body/sensor"))
        st.problem.add_goal(JR("gimbal_parent", 1.5, joint_path="/jointset/gimbal",
                               reaction_weights={"moment-y": 0.25}))
    return st


def _spline_knee(dynamics):
    return lambda reaction=True: configs.spline_knee_weld(2, dynamics=dynamics, reaction=reaction)


def _coupled(dynamics):
    def make(reaction=True):
        st = configs.double_pendulum_coupled(2, dynamics=dynamics)
        if reaction:
            st.problem.add_goal(JR("j1_child", 0.5, joint_path="j1", loads_frame="child"))
            st.problem.add_goal(JR("j0_parent", 1.0, joint_path="j0", reaction_measures=["force-y", "moment-z"]))
        return st
    return make


GAIT_PINS = ("hip_r", "hip_l", "ankle_r", "ankle_l", "back")


def _gait(reaction=True):
    """gait10dof18musc (muscles, ground-reaction forces) at N = 3 with the
    pelvis joint's and five pins' loads on the child in ground, and the right
    knee's in its child frame."""
    st = configs.gait10dof18musc(3)
    if reaction:
        for jn in ("ground_pelvis",) + GAIT_PINS:
            st.problem.add_goal(JR("load_" + jn, 0.01, joint_path=jn, loads_frame="child",
                                   expressed_in_frame_path="/ground"))
        st.problem.add_goal(JR("knee_reaction", 0.1, joint_path="knee_r", loads_frame="child"))
    return st


# case -> (study builder, "generic" to force the interpreter for g and J, muscle-free?)
CASES = {
    "pendulum_hs_2_explicit": (_pendulum(2, "hermite-simpson", "explicit"), "", True),
    "pendulum_hs_3_implicit": (_pendulum(3, "hermite-simpson", "implicit"), "", True),
    "pendulum_trap_3_explicit": (_pendulum(3, "trapezoidal", "explicit"), "", True),
    "pendulum_trap_2_implicit": (_pendulum(2, "trapezoidal", "implicit"), "", True),
    "gimbal_2": (_gimbal, "", True),
    "spline_knee_2_explicit": (_spline_knee("explicit"), "", True),
    "spline_knee_2_implicit": (_spline_knee("implicit"), "", True),
    "coupled_2_explicit": (_coupled("explicit"), "", True),
    "coupled_2_implicit": (_coupled("implicit"), "", True),
    "gait_3_generic": (_gait, "generic", False),
    "gait_3_generated": (_gait, "", False),
}
FREE = [c for c in CASES if CASES[c][2]]
MATRIX = [(c, fd) for c in FREE for fd in (("central", "forward", "backward") if c.startswith("pendulum")
                                           else ("central", "forward"))]
GAIT_MATRIX = [("gait_3_generic", "forward"), ("gait_3_generated", "forward"), ("gait_3_generated", "central")]


def _study(case, fd, reaction=True):
    st = CASES[case][0](reaction)
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
    """A random iterate (in implicit mode the accelerations are random too:
    not the solved ones).  spline_knee: the knee within 0.1 of the middle of a
    spline piece, so that every difference stencil of the checker stays on one
    piece.  gait: the muscle model's working range."""
    x = nlp.random_iterate(np.random.default_rng(17).uniform(-1, 1, nlp.n))
    G, NS, NC = nlp.G, nlp.NS, nlp.NC
    r = np.random.default_rng(18)
    if case.startswith("gait"):
        x[2:2 + NS * G] = r.uniform(0.05, 0.5, NS * G)
        x[2 + NS * G:2 + (NS + NC) * G] = r.uniform(0.05, 0.4, NC * G)
        x[0], x[1] = 0.3, 1.2
        return x
    x[0], x[1] = 0.05, 0.85
    S = x[2:2 + NS * G].reshape(G, NS)
    nq = nlp.NQ
    S[:, :nq] = r.uniform(-1.0, 1.0, (G, nq))
    S[:, nq:2 * nq] = r.uniform(-2.0, 2.0, (G, nq))
    if case.startswith("spline"):
        names = [c.name for c in st.problem.model.coordinates()]
        S[:, names.index("knee")] = -1.8 + 0.4 * r.integers(0, 4, G) + r.uniform(-0.1, 0.1, G)
    return x


def _grad_index(nlp, k, j):
    """x index of point input j (< NI - NSL) of grid point k."""
    G, NS, NC, NDV, NM, NSL = nlp.G, nlp.NS, nlp.NC, nlp.NDV, nlp.NM, nlp.NSL
    XM = 2 + (NS + NC) * G
    DB = XM + NM * G + NSL * nlp.opts.num_mesh_intervals
    if j < NS:
        return 2 + k * NS + j
    if j < NS + NC:
        return 2 + NS * G + k * NC + (j - NS)
    if j < NS + NC + NDV:
        return DB + k * NDV + (j - NS - NC)
    return XM + k * NM + (j - NS - NC - NDV)


@functools.lru_cache(maxsize=None)
def _base(case):
    """Per case, once: the iterate, the layout, the device's loads of every
    goal at every grid point and the DAE outputs there."""
    st = _study(case, "forward")
    nlp = _nlp(case, st)
    d = {"st": st, "model": st.problem.model, "ms": nlp.rep}
    d["grid"], d["quad"] = quadrature(nlp)
    x = d["x"] = _iterate(case, nlp, st)
    for k in ("G", "NS", "NC", "NDV", "NM", "NSL", "NI", "NQ", "n"):
        d[k] = getattr(nlp, k)
    d["implicit"] = bool(nlp.implicit)
    d["idx"] = np.array([[_grad_index(nlp, k, j) for j in range(nlp.NI - nlp.NSL)] for k in range(nlp.G)])
    d["P"] = nlp.point_inputs(x)
    d["t"] = x[0] + (x[1] - x[0]) * d["grid"]
    d["goals"] = [(g, gi) for gi, g in enumerate(st.problem.goals) if isinstance(g, JR)]
    d["loads"] = {g.name: nlp.joint_reaction(x, g.name) for g, _ in d["goals"]}
    d["dae"] = nlp.eval_dae(np.column_stack([d["t"], d["P"]]))
    nlp.close()
    return d


def _split(b, row):
    NS, NC, NDV, nq = b["NS"], b["NC"], b["NDV"], b["NQ"]
    q, u = row[:nq], row[nq:2 * nq]
    controls = row[NS:NS + NC]
    acc = row[NS + NC:NS + NC + nq] if b["implicit"] else None
    mult = row[NS + NC + NDV:NS + NC + NDV + b["NM"]]
    return q, u, controls, acc, mult


def _restated_L(b, row, t):
    """[L of every goal] by the restatement at one point's inputs: implicit
    dynamics reads the row's accelerations, explicit dynamics solves them."""
    q, u, controls, acc, mult = _split(b, row)
    ud = acc if b["implicit"] else solved_udot(b["model"], b["ms"], q, u, controls, mult, t)
    return np.array([reaction(b["model"], b["ms"], g, q, u, ud, t)[1] for g, _ in b["goals"]])


@functools.lru_cache(maxsize=None)
def _restated(case):
    """The restatement of a muscle-free case at its iterate: per goal and grid
    point L; of the weighted sum over the goals the slope (sixth-order central
    difference, step 1e-2) and the second and third derivatives (second
    differences, step 1e-3) along every direction."""
    b = _base(case)
    G, nd = b["G"], b["NI"] - b["NSL"]
    W = np.array([g.weight for g, _ in b["goals"]])
    L = np.array([_restated_L(b, b["P"][k], b["t"][k]) for k in range(G)]).T   # [goal, G]
    grad, d2, d3 = np.zeros((G, nd)), np.zeros((G, nd)), np.zeros((G, nd))
    dl = 1e-3
    for k in range(G):
        for j in range(nd):
            def val(a):
                row = b["P"][k].copy()
                row[j] += a
                return float(W @ _restated_L(b, row, b["t"][k]))
            grad[k, j] = _diff6(val)
            v = [val(a) for a in (0.0, dl, -dl, 2 * dl, -2 * dl)]
            d2[k, j] = abs(v[1] - 2.0 * v[0] + v[2]) / dl ** 2
            d3[k, j] = abs(v[3] - 2.0 * v[1] + 2.0 * v[2] - v[4]) / (2.0 * dl ** 3)
    return {"L": L, "W": W, "grad": grad, "d2": d2, "d3": d3}


@functools.lru_cache(maxsize=None)
def _evaluated(case, fd):
    """Everything the GPU tests of one (case, scheme) read, computed once: with
    the goals f, the terms, grad f (twice); the same study without them."""
    b = _base(case)
    x = b["x"]
    st = _study(case, fd)
    nlp = _nlp(case, st)
    d = {"st": st, "h": st.solver.fd_step if st.solver.fd_step > 0 else 1e-8}
    assert nlp.n == b["n"]
    d["f"], d["terms"], d["grad"] = nlp.eval_f(x), nlp.objective_terms(x), nlp.eval_grad_f(x)
    d["f2"], d["grad2"] = nlp.eval_f(x), nlp.eval_grad_f(x)
    nlp.close()
    nlp0 = _nlp(case, _study(case, fd, False))
    assert nlp0.n == b["n"]
    d["f0"], d["grad0"], d["terms0"] = nlp0.eval_f(x), nlp0.eval_grad_f(x), nlp0.objective_terms(x)
    nlp0.close()
    return d


# ---- CPU --------------------------------------------------------------------

def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / (np.abs(want).max() + 1e-300))


def test_restatement_against_closed_forms():
    """A single pendulum at (q, u, udot): mass 1 at distance 1 from the pin,
    inertia 1 about its centre, gravity -g y.  On the child at the pin, in
    ground: force = m (a_c - g), moment z = (I + m) udot + m g cos q.  A mass on
    a slider along x with gravity (3, -2, 0.5): force = m (udot x - g), no
    moment about its centre.  To 1e-12 relative."""
    m = configs.n_link_pendulum(1)
    g = 9.80665
    for q, u, ud in ((0.3, -1.7, 2.9), (-2.2, 4.1, -0.6), (1.4, 0.0, 0.0)):
        goal = JR("r", joint_path="j0", loads_frame="child", expressed_in_frame_path="/ground")
        r, L = reaction(m, None, goal, np.array([q]), np.array([u]), np.array([ud]), 0.0)
        ac = ud * np.array([-math.sin(q), math.cos(q), 0.0]) - u * u * np.array([math.cos(q), math.sin(q), 0.0])
        want = np.array([0.0, 0.0, 2.0 * ud + g * math.cos(q), ac[0], ac[1] + g, ac[2]])
        assert _rel(r, want) <= 1e-12, (r, want)
        assert abs(L - float(want @ want) / g) <= 1e-12 * (abs(L) + 1.0)
        # on the parent (ground, at the same point): the opposite load
        rp, _ = reaction(m, None, JR("r", joint_path="j0", expressed_in_frame_path="/ground"), np.array([q]),
                         np.array([u]), np.array([ud]), 0.0)
        assert _rel(rp, -want) <= 1e-12
        # expressed in the body: rotated by -q about z
        rb, _ = reaction(m, None, JR("r", joint_path="j0", loads_frame="child"), np.array([q]), np.array([u]),
                         np.array([ud]), 0.0)
        c, s = math.cos(q), math.sin(q)
        Rt = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
        assert _rel(rb, np.concatenate([Rt @ want[:3], Rt @ want[3:]])) <= 1e-12
        # the restated inverse dynamics: tau = (I + m) udot + m g cos q
        tau = generalized_forces(m, None, np.array([q]), np.array([u]), np.array([ud]), 0.0)
        assert abs(tau[0] - want[2]) <= 1e-12 * (abs(want[2]) + 1.0)
    st = configs.sliding_mass(2)
    sm = st.problem.model
    sm.gravity = (3.0, -2.0, 0.5)
    goal = JR("r", joint_path="slider", loads_frame="child")
    for q, u, ud in ((0.7, -1.2, 3.3), (-4.0, 2.0, -0.25)):
        r, L = reaction(sm, None, goal, np.array([q]), np.array([u]), np.array([ud]), 0.0)
        want = np.array([0.0, 0.0, 0.0, 2.0 * (ud - 3.0), 4.0, -1.0])
        assert _rel(r, want) <= 1e-12, (r, want)
        assert abs(L - float(want @ want) / (2.0 * math.sqrt(3.0 ** 2 + 2.0 ** 2 + 0.5 ** 2))) <= 1e-12 * (L + 1.0)
        ud2 = solved_udot(sm, None, np.array([q]), np.array([u]), np.array([1.7]), np.zeros(0), 0.0)
        assert abs(ud2[0] - (1.7 / 2.0 + 3.0)) <= 1e-12


def _terms(st, gi):
    rep = st.problem.create_rep()
    G = rep.struct.goals[gi]
    tb = G.term_begin
    return (G, list(rep._gidx[tb:tb + G.term_count]), list(rep._gcol[tb:tb + G.term_count]),
            np.array(rep._gw[tb:tb + G.term_count]), rep)


def test_lowering_defaults_and_each_property():
    """The sixteen terms of include/mocohip.h: defaults (parent frame, R_PF,
    all six weights 1, total mass x |gravity|), the child frame (R_BM), an
    expressed-in offset frame, body and ground, the measures' subset and
    weights, and the denominator without gravity."""
    st = configs.gimbal_frame_tracking(2)
    m = st.problem.model
    st.problem.add_goal(JR("d", 2.5, joint_path="gimbal"))
    G, gidx, gcol, gw, rep = _terms(st, len(st.problem.goals) - 1)
    assert (G.kind, G.term_count, G.weight, G.table) == (abi.MH_GOAL_JOINT_REACTION, 16, 2.5, -1) and G.kind == 14
    b = rep.compiled.body_index["body"]
    assert gidx == [b] * 16
    assert gcol == [-1] * 9 + [-1] * 6 + [0]   # the parent is ground
    assert np.array_equal(gw[:9].reshape(3, 3), body_fixed_xyz((0, 0, -math.pi / 2)))
    assert np.array_equal(gw[9:15], np.ones(6))
    assert gw[15] == 1.0 * math.sqrt((0.0 * 0.0 + 9.80665 * 9.80665) + 0.0 * 0.0)
    st.problem.goals[-1] = JR("c", joint_path="/jointset/gimbal", loads_frame="child")
    G, gidx, gcol, gw, rep = _terms(st, len(st.problem.goals) - 1)
    assert gcol == [b] * 9 + [-1] * 6 + [1] and np.array_equal(gw[:9].reshape(3, 3), np.eye(3))
    st.problem.goals[-1] = JR("e", joint_path="gimbal", expressed_in_frame_path="/bodyset/body/sensor",
                              reaction_measures=["force-z", "moment-y"], reaction_weights={"moment-y": 4.0,
                                                                                          "force-x": 9.0})
    G, gidx, gcol, gw, rep = _terms(st, len(st.problem.goals) - 1)
    assert gcol == [b] * 9 + [-1] * 6 + [0]
    assert np.array_equal(gw[:9].reshape(3, 3), body_fixed_xyz((0.4, -0.7, 1.1)))
    assert list(gw[9:15]) == [0.0, 4.0, 0.0, 0.0, 0.0, 1.0]
    for path, e in (("/ground", -1), ("/bodyset/body", b), ("body", b)):
        st.problem.goals[-1] = JR("e", joint_path="gimbal", expressed_in_frame_path=path)
        G, gidx, gcol, gw, rep = _terms(st, len(st.problem.goals) - 1)
        assert gcol[:9] == [e] * 9 and np.array_equal(gw[:9].reshape(3, 3), np.eye(3))
    # a weld is a joint like any other; two bodies: the total mass
    st = configs.spline_knee_weld(2)
    G, gidx, gcol, gw, rep = _terms(st, len(st.problem.goals) - 1)
    bi = rep.compiled.body_index
    assert gidx == [bi["brace"]] * 16 and gcol[0] == bi["shank"] and gcol[15] == 0
    assert np.array_equal(gw[:9].reshape(3, 3), body_fixed_xyz((0.1, -0.2, 0.3)))
    assert gw[15] == ((2.0 + 1.5) + 0.4) * 9.80665
    # no gravity: the total mass
    st = configs.sliding_mass(2)
    st.problem.add_goal(JR("s", joint_path="slider"))
    assert _terms(st, 1)[3][15] == 2.0
    st.problem.model.gravity = (0.0, 1e-15, 0.0)   # below eps^0.875
    assert _terms(st, 1)[3][15] == 2.0
    st.problem.model.gravity = (0.0, 1e-13, 0.0)
    assert _terms(st, 1)[3][15] == 2.0 * 1e-13


def _bad_goals():
    return [
        (JR("g"), "Expected a joint path, but property joint_path is empty."),
        (JR("g", joint_path="j1", reaction_measures=["force-x", "torque-x"]),
         "Reaction measure 'torque-x' not recognized."),
        (JR("g", joint_path="j1", loads_frame="both"),
         "Property 'loads_frame' (in object 'g' of type MocoJointReactionGoal) has invalid value both; "
         "expected one of the following:  child  parent."),
        (JR("g", joint_path="j7"), "no joint 'j7' in the model"),
        (JR("g", joint_path="j1", expressed_in_frame_path="/bodyset/b9"), "no frame '/bodyset/b9' in the model"),
        (JR("g", joint_path="j1", reaction_weights={"force-y": -1.0}), "negative weight -1"),
    ]


def test_lowering_reports_the_reference_errors(tmp_path):
    """The reference's messages (MocoJointReactionGoal.cpp:40-41, :82-84,
    checkPropertyInSet), from problem.py and from mh_build alike; prescribed
    kinematics and MocoParameters are refused by both."""
    for goal, msg in _bad_goals():
        st = configs.double_pendulum_joint_reaction(2, reaction=False)
        st.problem.add_goal(goal)
        with pytest.raises(ValueError) as e:
            st.problem.create_rep()
        assert msg in str(e.value)
        desc = tmp_path / "bad.mhdesc"
        write_description(st, str(desc))
        r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "bad.tape")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (msg, r.stderr)
    st = configs.gait10dof18musc_inverse(2)
    st.problem.add_goal(JR("g", joint_path="knee_r"))
    with pytest.raises(NotImplementedError, match="MocoJointReactionGoal with prescribed kinematics"):
        st.problem.create_rep()
    st = configs.oscillator_mass(2)
    st.problem.add_goal(JR("g", joint_path=st.problem.model.joints[0].name))
    with pytest.raises(NotImplementedError, match="MocoJointReactionGoal with MocoParameters"):
        st.problem.create_rep()
    for st in (st, ):
        desc = tmp_path / "par.mhdesc"
        write_description(st, str(desc))
        r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "par.tape")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and "MocoJointReactionGoal with MocoParameters" in r.stderr, r.stderr


BUILDER_CASES = {
    "pendulum": lambda: configs.double_pendulum_joint_reaction(2),
    "gimbal": _gimbal,
    "spline_knee_weld": lambda: configs.spline_knee_weld(2, dynamics="implicit"),
    "coupled": _coupled("explicit"),
    "cart": lambda: configs.cart_welded_payload(5),
    "inverted_pendulum": lambda: configs.inverted_pendulum(4, "reaction"),
    "gait": _gait,
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    problem.py; the description carries one goal joint_reaction record per goal."""
    st = BUILDER_CASES[name]()
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    n = sum(isinstance(g, JR) for g in st.problem.goals)
    assert n >= 1 and sum(ln.startswith("goal joint_reaction ") for ln in desc.read_text().splitlines()) == n
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


def _bad_problems():
    """(study builder, mutation of its mh_problem, message, error code).  In
    the pendulum study goal 1 is the first joint-reaction goal."""
    pend = lambda: configs.double_pendulum_joint_reaction(2)   # noqa: E731
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

    def presc_study():   # the joint-reaction goals first, and a table to prescribe from
        st = configs.double_pendulum_joint_reaction(2, dynamics="implicit")   # (prescribed kinematics needs it)
        st.problem.goals = st.problem.goals[1:] + st.problem.goals[:1]
        st.problem.model.add_table(DataTable("kin", np.linspace(0.0, 1.0, 4), {"a": np.zeros(4)}, degree=1))
        return st

    I, U = abi.MH_ERR_INVALID, abi.MH_ERR_UNSUPPORTED
    return [
        (pend, setg(term_count=15), "joint reaction goal needs 16 terms", I),
        (pend, setg(term_count=17), "joint reaction goal needs 16 terms", I),
        (pend, seti("goal_index", 7, 0), "a joint reaction goal's terms name different bodies", I),
        (pend, seti("goal_index", 15, 0), "a joint reaction goal's terms name different bodies", I),
        (pend, lambda p: [seti("goal_index", k, 2)(p) for k in range(16)], "child body 2 out of range", I),
        (pend, lambda p: [seti("goal_index", k, -1)(p) for k in range(16)], "child body -1 out of range", I),
        (pend, lambda p: [seti("goal_column", k, 2)(p) for k in range(9)], "expressed-in body 2 out of range", I),
        (pend, lambda p: [seti("goal_column", k, -2)(p) for k in range(9)], "expressed-in body -2 out of range", I),
        (pend, seti("goal_column", 4, 0), "name different expressed-in bodies", I),
        (pend, seti("goal_weight", 12, -0.5), "negative joint reaction measure weight", I),
        (pend, seti("goal_column", 15, 2), "loads frame 2 is neither 0 (parent) nor 1 (child)", I),
        (pend, seti("goal_column", 15, -1), "loads frame -1 is neither 0 (parent) nor 1 (child)", I),
        (pend, seti("goal_weight", 15, 0.0), "is not positive and finite", I),
        (pend, seti("goal_weight", 15, -3.0), "is not positive and finite", I),
        (pend, seti("goal_weight", 15, math.inf), "is not positive and finite", I),
        (pend, seti("goal_weight", 15, math.nan), "is not positive and finite", I),
        (pend, setg(kind=13), "unknown kind 13", I),
        (presc_study, prescribe, "joint reaction goal with prescribed kinematics", U),
        (pend, parameter, "joint reaction goal with MocoParameters", U),
    ]


def test_layout_query_accepts_the_goal_and_refuses_what_create_refuses():
    """mh_get_nlp_info_for (host only): the goal changes no layout count;
    every refusal comes with its code and message; kind 13 is still unknown."""
    lib = abi.load_mocohip()
    for case in ("pendulum_hs_2_explicit", "pendulum_trap_2_implicit", "gimbal_2", "spline_knee_2_implicit",
                 "coupled_2_explicit", "gait_3_generated"):
        (rc, a, _), (rc0, b, _) = _info(CASES[case][0](True)), _info(CASES[case][0](False))
        assert rc == 0 and rc0 == 0, lib.mh_last_error().decode()
        assert (a.n, a.m, a.nnz_jac_g, a.num_grid_points, a.num_states, a.num_controls) == \
            (b.n, b.m, b.nnz_jac_g, b.num_grid_points, b.num_states, b.num_controls)
    for make, mutate, msg, code in _bad_problems():
        rc, _, _ = _info(make(), mutate)
        assert rc == code and msg in lib.mh_last_error().decode(), (msg, rc, lib.mh_last_error().decode())
        assert lib.mh_last_error().decode().startswith("goal ")   # the message names the goal


# ---- GPU --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", FREE)
def test_loads_against_the_restatement(case):
    """mh_eval_joint_reaction at every grid point of the iterate against the
    restatement, per component within 1e-10 (|want| + 1).  Implicit dynamics:
    the iterate's (random) accelerations.  Explicit dynamics: the restatement
    is fed the udot that mh_eval_dae solves, and the restatement's own forward
    dynamics must give that udot."""
    b = _base(case)
    worst = 0.0
    for k in range(b["G"]):
        q, u, controls, acc, mult = _split(b, b["P"][k])
        ud = acc if b["implicit"] else b["dae"][k, :b["NQ"]]
        if not b["implicit"]:
            mine = solved_udot(b["model"], b["ms"], q, u, controls, mult, b["t"][k])
            assert np.abs(mine - ud).max() <= 1e-10 * (np.abs(ud).max() + 1.0)
        for g, _ in b["goals"]:
            want, _ = reaction(b["model"], b["ms"], g, q, u, ud, b["t"][k])
            got = b["loads"][g.name][k]
            err = np.abs(got - want) / (np.abs(want) + 1.0)
            worst = max(worst, float(err.max()))
            assert (err <= 1e-10).all(), (case, k, g.name, got, want)
            assert np.abs(want).max() > 1e-3
    print(f"{case}: worst |load - restated| / (|restated| + 1) = {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("dyn", ["pendulum_hs_2", "spline_knee_2", "coupled_2"])
def test_explicit_matches_implicit_fed_the_explicit_udot(dyn):
    """The explicit context's loads at its iterate equal, within 1e-10 (|want|
    + 1), those of an implicit context of the same model whose acceleration
    inputs are the udot taken from the explicit context's mh_eval_dae."""
    case = dyn + "_explicit"
    b = _base(case)
    other = {"pendulum_hs_2": lambda r=True: configs.double_pendulum_joint_reaction(
        2, "hermite-simpson", "central", "implicit", r), "spline_knee_2": _spline_knee("implicit"),
        "coupled_2": _coupled("implicit")}[dyn]
    from mocohip.solver import HipNLP
    st = other()
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    NS, NC, nq = b["NS"], b["NC"], b["NQ"]
    assert nlp.NS == NS and nlp.NC == NC and nlp.NDV >= nq
    rows = np.zeros((b["G"], 1 + nlp.NI))
    rows[:, 0] = b["t"]
    rows[:, 1:1 + NS + NC] = b["P"][:, :NS + NC]
    rows[:, 1 + NS + NC:1 + NS + NC + nq] = b["dae"][:, :nq]
    rows[:, 1 + NS + NC + nlp.NDV:1 + NS + NC + nlp.NDV + nlp.NM] = b["P"][:, NS + NC + b["NDV"]:
                                                                      NS + NC + b["NDV"] + b["NM"]]
    for gi, g in enumerate(st.problem.goals):
        if not isinstance(g, JR):
            continue
        got, want = b["loads"][g.name], nlp.eval_joint_reaction(gi, rows)
        assert (np.abs(got - want) <= 1e-10 * (np.abs(want) + 1.0)).all(), (g.name, got, want)
    nlp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gait_3_generic", "gait_3_generated"])
def test_gait_momentum_balance_and_mobility_forces(case):
    """gait10dof18musc with muscles and ground-reaction forces, udot from
    mh_eval_dae.  The ground-pelvis load equals the restatement's whole-body
    momentum balance with the ground-reaction forces: the muscle forces cancel.
    At every pin whose coordinate no moving path point reads, the joint axis
    dotted into the load's moment about the joint centre equals the applied
    mobility force (the reserve actuator's).  The generated back end serves g
    and J of one case; the loads are the interpreter's in both, bit for bit."""
    b = _base(case)
    model, nq = b["model"], b["NQ"]
    qidx = model.coordinate_index()
    assert all(p.body != "ground" for mu in model.muscles for p in mu.points)
    moving = {f.coord for mu in model.muscles for p in mu.points for f in (p.fx, p.fy, p.fz) if f is not None}
    ctrl = {a.coordinate: (i, a.optimal_force) for i, a in enumerate(model.actuators) if not hasattr(a, "points")}
    checked = 0
    for k in range(b["G"]):
        q, u, controls, _, _ = _split(b, b["P"][k])
        ud = b["dae"][k, :nq]
        rates, mot, pose = momentum_rates(model, b["ms"], q, u, ud, b["t"][k])
        F = sum(rates.values())
        pelvis = next(j for j in model.joints if j.name == "ground_pelvis")
        o = mot["pelvis"][1] + mot["pelvis"][0] @ np.asarray(pelvis.loc_in_child, float)
        want = np.concatenate([F[:3] - np.cross(o, F[3:]), F[3:]])
        got = b["loads"]["load_ground_pelvis"][k]
        assert (np.abs(got - want) <= 1e-10 * (np.abs(want) + 1.0)).all(), (k, got, want)
        for jn in GAIT_PINS:
            j = next(j for j in model.joints if j.name == jn)
            own = pose[j.child][2][len(pose[j.parent][2]):]
            if len(own) != 1 or not own[0][2] or j.coordinates[0].name in moving:
                continue
            s, dv, _, a, _ = own[0]
            i, opt = ctrl[j.coordinates[0].name]
            applied = controls[i] * opt
            got = dv * float(a @ b["loads"]["load_" + jn][k][:3])
            scale = np.abs(b["loads"]["load_" + jn][k][:3]).max()
            assert abs(got - applied) <= 1e-10 * (scale + abs(applied) + 1.0), (jn, k, got, applied)
            checked += 1
    assert checked >= 3 * b["G"]
    other = _base("gait_3_generic" if case == "gait_3_generated" else "gait_3_generated")
    for name, v in b["loads"].items():
        assert np.array_equal(v, other["loads"][name])


def _check_terms(case, fd, want_L):
    b, d = _base(case), _evaluated(case, fd)
    x = b["x"]
    total, gis = 0.0, []
    for j, (goal, gi) in enumerate(b["goals"]):
        want = goal.weight * (x[1] - x[0]) * float(b["quad"] @ want_L[j])
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
def test_objective_against_the_restatement(case, fd):
    """Each goal's entry of mh_eval_objective_terms and f - f0: weight *
    duration * sum_k quad_k L_k of the restatement within 1e-10 (|want| + 1);
    the other goals' terms are those of the study without the goal, bit for
    bit; two evaluations give the same bits."""
    _check_terms(case, fd, _restated(case)["L"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", GAIT_MATRIX)
def test_gait_objective_from_the_probed_loads(case, fd):
    """gait10dof18musc: the terms and f - f0 from the integrand of the loads
    that mh_eval_joint_reaction gives (checked against the momentum balance
    above), the other goals' terms bit-identical, determinism."""
    b = _base(case)
    L = np.array([[float(resolve(b["model"], g)[4] @ (r * r)) / resolve(b["model"], g)[5]
                   for r in b["loads"][g.name]] for g, _ in b["goals"]])
    _check_terms(case, fd, L)


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_gradient_against_the_restatement(case, fd):
    """mh_eval_grad_f minus the gradient of the study without the goals over
    every direction (t0, tf, states, controls, accelerations, multipliers),
    with test_frame_tracking's tolerance model unchanged: per quotient the
    measured value error over h plus the scheme's truncation (h / 2 |L''| or
    h^2 / 6 |L'''| from second differences of the restatement, doubled); plus
    64 eps |grad0|.  The integrand does not depend on t here (no external
    loads): its t0 / tf quotients are exact zeros."""
    b, r, d = _base(case), _restated(case), _evaluated(case, fd)
    x, G, h = b["x"], b["G"], d["h"]
    dur, quad, g = x[1] - x[0], b["quad"], b["grid"]
    L = r["W"] @ r["L"]
    diff = d["grad"] - d["grad0"]
    rel = max(abs(d["terms"][gi] - goal.weight * dur * float(quad @ r["L"][j]))
              / (abs(goal.weight * dur * float(quad @ r["L"][j])) + 1.0)
              for j, (goal, gi) in enumerate(b["goals"]))   # measured value error, <= 1e-10
    dv = rel * (np.abs(L) + 1.0) + 64 * EPS * (np.abs(L).max() + 1.0)
    trunc = 2.0 * (h * h / 6.0 * r["d3"] if fd == "central" else h / 2.0 * r["d2"])
    worst = 0.0
    for k in range(G):
        for s in range(b["NI"] - b["NSL"]):
            scale = dur * quad[k]
            want = scale * r["grad"][k, s]
            i = b["idx"][k, s]
            tol = scale * (1e-8 * abs(r["grad"][k, s]) + 8 * dv[k] / h + trunc[k, s]) + 64 * EPS * abs(d["grad0"][i])
            worst = max(worst, abs(diff[i] - want) / tol)
            assert abs(diff[i] - want) <= tol, (k, s, diff[i], want, tol)
    acc = float(quad @ L)
    for c in (0, 1):
        want = -acc if c == 0 else acc
        tol = 1e-10 * (abs(acc) + 1.0) + 64 * EPS * abs(d["grad0"][c])
        worst = max(worst, abs(diff[c] - want) / tol)
        assert abs(diff[c] - want) <= tol, (c, diff[c], want, tol)
    print(f"{case} {fd}: worst |grad f - ref| / tol = {worst:.3e}")
    moved = np.abs(diff[b["idx"]]).max(axis=0)
    nq, na = b["NQ"], b["NS"] + b["NC"]
    assert (moved[:2 * nq] > 0.0).all()                  # every coordinate and speed
    if b["implicit"]:   # the accelerations; controls and multipliers reach the load only through udot
        assert (moved[na:na + nq] > 0.0).all()
        assert (moved[b["NS"]:na] == 0.0).all() and (moved[na + b["NDV"]:] == 0.0).all()
    else:
        assert (moved[b["NS"]:] > 0.0).all()             # every control and multiplier
    touched = np.zeros(b["n"], bool)
    touched[[0, 1]] = True
    touched[b["idx"].ravel()] = True
    assert np.array_equal(d["grad"][~touched], d["grad0"][~touched], equal_nan=True)   # the slacks


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", GAIT_MATRIX)
def test_gait_exact_zeros(case, fd):
    """An excitation of a muscle with activation dynamics enters the DAE only
    through that muscle's activation derivative: the load does not move, the
    quotient is an exact zero and the entry keeps the bits of the study
    without the goals.  The coordinates, speeds and activations do move."""
    b, d = _base(case), _evaluated(case, fd)
    model = b["model"]
    diff_bits = d["grad"] != d["grad0"]
    exc = [i for i, a in enumerate(model.actuators) if hasattr(a, "points") and not a.ignore_activation_dynamics]
    assert len(exc) > 0
    for k in range(b["G"]):
        for i in exc:
            j = b["idx"][k, b["NS"] + i]
            assert d["grad"][j] == d["grad0"][j] and not diff_bits[j]
        assert diff_bits[b["idx"][k, :b["NS"]]].all()
    assert diff_bits[0] and diff_bits[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pendulum_hs_3_implicit", "coupled_2_explicit", "gait_3_generated"])
def test_shards_sum_to_the_whole(case):
    """mh_eval_f_partial / mh_eval_grad_f_partial over 2 shards, with the
    bounds of test_angular_velocity_tracking's shard test."""
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
    mh_eval_joint_reaction refuses a goal that is not of kind 14."""
    from mocohip.solver import HipNLP
    for make, mutate, msg, _ in _bad_problems():
        st = make()
        rep = st.problem.create_rep()
        mutate(rep.struct)
        with pytest.raises(RuntimeError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            HipNLP(rep, st.solver.options())
    st = configs.double_pendulum_joint_reaction(2)
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    rows = np.zeros((1, 1 + nlp.NI))
    for goal in (0, -1, 4, 99):
        with pytest.raises(RuntimeError, match="is not a joint reaction goal"):
            nlp.eval_joint_reaction(goal, rows)
    with pytest.raises(ValueError, match="no goal 'nothing'"):
        nlp.joint_reaction(np.zeros(nlp.n), "nothing")
    assert nlp.eval_joint_reaction(1, rows).shape == (1, 6)
    nlp.close()


@pytest.mark.gpu
def test_cart_with_a_welded_payload_falls_freely():
    """Solve 1 (the slider stand-in for testMocoGoals.cpp:364-411): minimizing
    force-x of the weld between cart and payload under gravity (10, 0, 0) along
    the slider gives free fall: |control| <= 1e-3 (the reference's 1e-4
    relative on its magnitude 10), objective <= 1e-6, final position 5 and
    final speed 10 within 1e-3."""
    sol = configs.cart_welded_payload(5).solve()
    print(f"cart: {sol.metadata['num_iterations']} iterations, status {sol.metadata.get('status')}, objective "
          f"{sol.metadata['objective']}, max |control| {np.abs(sol.controls).max():.3e}, final "
          f"{sol.states[-1]}")
    assert sol.metadata["success"] == "true", sol.metadata
    assert np.abs(sol.controls).max() <= 1e-3
    assert float(sol.metadata["objective"]) <= 1e-6
    assert abs(sol.get_state("/jointset/slider/x/value")[-1] - 5.0) <= 1e-3
    assert abs(sol.get_state("/jointset/slider/x/speed")[-1] - 10.0) <= 1e-3


@pytest.mark.gpu
def test_inverted_pendulum_effort_against_reaction():
    """Solve 2 (exampleMinimizeJointReaction.m:44-106 at N = 20): once with
    MocoControlGoal, once with MocoJointReactionGoal on the pin; both converge.
    Each solution's reaction integral is recomputed through the new entry (on
    the reaction study's context) and its effort from its controls: the
    reaction-goal solution has the smaller reaction integral, the effort
    solution the smaller effort."""
    N = 20
    effort = configs.inverted_pendulum(N, "effort").solve()
    reaction_sol = configs.inverted_pendulum(N, "reaction").solve()
    for name, s in (("effort", effort), ("reaction", reaction_sol)):
        print(f"{name}: {s.metadata['num_iterations']} iterations, status {s.metadata.get('status')}, "
              f"objective {s.metadata['objective']}")
    assert effort.metadata["success"] == "true", effort.metadata
    assert reaction_sol.metadata["success"] == "true", reaction_sol.metadata
    st = configs.inverted_pendulum(N, "reaction")
    nlp = st.create_nlp()
    _, quad = quadrature(nlp)
    den = 1.0 * 9.80665

    def integrals(sol):
        loads = nlp.joint_reaction(sol, "reaction")
        assert loads.shape == (nlp.G, 6)
        dur = sol.time[-1] - sol.time[0]
        return (dur * float(quad @ (loads * loads).sum(axis=1)) / den,
                dur * float(quad @ (sol.controls[:, 0] ** 2)))
    re, ee = integrals(effort)
    rr, er = integrals(reaction_sol)
    x = reaction_sol.to_iterate(nlp)
    assert abs(nlp.eval_f(x) - rr) <= 1e-10 * (rr + 1.0)
    nlp.close()
    print(f"reaction integral: effort solution {re:.6g}, reaction solution {rr:.6g}; "
          f"effort: effort solution {ee:.6g}, reaction solution {er:.6g}")
    assert rr < re and ee < er
