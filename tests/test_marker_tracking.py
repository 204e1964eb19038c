"""MocoMarkerTrackingGoal evaluated by a device kinematics kernel
(MocoMarkerTrackingGoal.{h,cpp}; include/mocohip.h MH_GOAL_MARKER_TRACKING;
k_marker_tracking).

The checker is a NumPy restatement: the forward kinematics of
tests/test_frame_distance.py over the Python Model, the reference read from
the compiled table's piecewise polynomial, the integrand
sum_m w_m |p_G(marker m; q) - ref_m(t)|^2 and its analytic gradient along the
coordinates and the time.  It does not call the product-side helper that
synthesizes marker data (Model.marker_locations_in_ground).

CPU: the restatement against closed forms, the lowering (Python and the C++
builder, byte-identical tapes; every reference error) and the host-only layout
query.  GPU: f, the goal's objective term and grad f against the restatement,
exact zeros, nothing else moving, determinism, shards, refusals, and the
reference's example (exampleMarkerTracking.cpp) solved."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _lanes
from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.problem import MarkersReference, MocoMarkerTrackingGoal
from mocohip.tape import write_tape
from test_frame_distance import forward_kinematics, station

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_BUILD = os.path.join(ROOT, "opensim-moco_amd", "csrc", "build", "mh_build")
EPS = np.finfo(float).eps


# ---- the restatement --------------------------------------------------------

def table_value(model_struct, ti, col, t):
    """Value and time derivative of column col of model table ti at t: the
    segment that holds t (the end segments extrapolate), Horner in t - break."""
    T = model_struct.tables[ti]
    br = np.array([model_struct.table_breaks[T.break_begin + i] for i in range(T.nseg + 1)])
    s = 0 if t <= br[0] else T.nseg - 1 if t >= br[-1] else int(np.searchsorted(br, t, side="right") - 1)
    n = T.degree + 1
    cf = [model_struct.table_coefs[T.coef_begin + (s * T.ncol + col) * n + k] for k in range(n)]
    dt = t - br[s]
    v = sum(c * dt ** k for k, c in enumerate(cf))
    dv = sum(k * c * dt ** (k - 1) for k, c in enumerate(cf) if k > 0)
    return v, dv


def tracked_markers(st, rep):
    """[(body, location, weight, table, (x, y, z columns))] of the study's
    marker-tracking goal, resolved here: a label is a component path, else a
    name in the marker set; weights by reference index."""
    goal = next(g for g in st.problem.goals if isinstance(g, MocoMarkerTrackingGoal))
    model, ref = st.problem.model, goal.markers_reference
    ti = rep.compiled.table_index[ref.name]
    cols = rep.compiled.table_columns[ref.name]
    out = []
    for i, label in enumerate(ref.labels):
        mk = model.markers.get(label) or next((m for m in model.markers.values() if m.name == label), None)
        if mk is None:
            assert goal.allow_unused_references
            continue
        out.append((mk.body, tuple(mk.location), ref.weights()[i], ti,
                    tuple(cols.index(f"{label}_{c}") for c in (1, 2, 3))))
    return goal, out


def integrand(model, model_struct, markers, q, t):
    """L(t, q), dL/dq [nq], dL/dt."""
    nq = len(q)
    pose = forward_kinematics(model, q)
    L, dq, dt = 0.0, np.zeros(nq), 0.0
    for body, loc, w, ti, cols in markers:
        P, dP = station(model, pose, body, loc, nq)
        rv = [table_value(model_struct, ti, c, t) for c in cols]
        d = P - np.array([v for v, _ in rv])
        L += w * (d @ d)
        dq += w * 2.0 * (d @ dP)
        dt -= w * 2.0 * (d @ np.array([dv for _, dv in rv]))
    return L, dq, dt


def quadrature(nlp):
    """The grid's quadrature weights over [0, 1] (Hermite-Simpson: 1/6, 2/3,
    1/6 of each mesh interval; trapezoidal: 1/2, 1/2)."""
    g = _lanes.grid(nlp)
    w = np.zeros(nlp.G)
    if nlp.opts.transcription == abi.MH_HERMITE_SIMPSON:
        for i in range(0, nlp.G - 1, 2):
            dm = g[i + 2] - g[i]
            w[i] += dm / 6; w[i + 1] += 2 * dm / 3; w[i + 2] += dm / 6
    else:
        for i in range(nlp.G - 1):
            dm = g[i + 1] - g[i]
            w[i] += dm / 2; w[i + 1] += dm / 2
    return g, w


def chain_coordinates(model, bodies):
    qidx = model.coordinate_index()
    parent = {j.child: j for j in model.joints}
    out = set()
    for b in bodies:
        while b != "ground":
            out.update(qidx[c.name] for c in parent[b].coordinates)
            b = parent[b].parent
    return sorted(out)


# ---- the studies ------------------------------------------------------------

CASES = {
    "pendulum_hs_2": (lambda: configs.double_pendulum_marker_tracking(2, "hermite-simpson"), None),
    "pendulum_hs_3": (lambda: configs.double_pendulum_marker_tracking(3, "hermite-simpson"), None),
    "pendulum_trapezoidal_2": (lambda: configs.double_pendulum_marker_tracking(2, "trapezoidal"), None),
    "pendulum_trapezoidal_3": (lambda: configs.double_pendulum_marker_tracking(3, "trapezoidal"), None),
    "gait_generated": (lambda: configs.gait10dof18musc_marker_track_few(3), "generated"),
    "gait_generic": (lambda: configs.gait10dof18musc_marker_track_few(3), "generic"),
}
FDS = ("forward", "backward", "central")
MATRIX = [(c, fd) for c in CASES for fd in FDS]


def _study(case, fd, goal=True):
    st = CASES[case][0]()
    st.solver.optim_finite_difference_scheme = fd
    if not goal:
        st.problem.goals = [g for g in st.problem.goals if not isinstance(g, MocoMarkerTrackingGoal)]
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


def _iterate(nlp, muscles):
    x = nlp.random_iterate(np.random.default_rng(7).uniform(-1, 1, nlp.n))
    if muscles:   # the muscle model's working range (tests/test_gpu_parity.py)
        G, NS, NC = nlp.G, nlp.NS, nlp.NC
        r = np.random.default_rng(8)
        x[2:2 + NS * G] = r.uniform(0.05, 0.5, NS * G)
        x[2 + NS * G:2 + (NS + NC) * G] = r.uniform(0.05, 0.4, NC * G)
    return x


@functools.lru_cache(maxsize=None)
def _restated(case):
    """The restatement of one case at its iterate, computed once (it does not
    depend on the finite-difference scheme): per grid point L, dL/dq, dL/dt
    and the second and third derivatives along every direction from second
    differences of the restatement (step 1e-3)."""
    st = _study(case, "forward")
    rep = st.problem.create_rep()
    goal, markers = tracked_markers(st, rep)
    model = st.problem.model
    nq = rep.nq
    d = {"goal": goal, "markers": markers, "gi": st.problem.goals.index(goal)}
    nlp = _nlp(case, st)
    x = _iterate(nlp, case.startswith("gait"))
    d["x"], d["G"], d["NS"], d["n"] = x, nlp.G, nlp.NS, nlp.n
    d["grid"], d["quad"] = quadrature(nlp)
    nlp.close()
    G, NS = d["G"], d["NS"]
    S = x[2:2 + NS * G].reshape(G, NS)
    t = (x[1] - x[0]) * d["grid"] + x[0]
    L, dq, dt = np.zeros(G), np.zeros((G, nq)), np.zeros(G)
    d2, d3 = np.zeros((G, nq + 1)), np.zeros((G, nq + 1))   # direction nq: the time
    dl = 1e-3
    f = lambda q, tt: integrand(model, rep.struct.model, markers, q, tt)
    for k in range(G):
        q = S[k, :nq].copy()
        L[k], dq[k], dt[k] = f(q, t[k])
        for s in range(nq + 1):
            qp, qm, tp, tm = q.copy(), q.copy(), t[k], t[k]
            if s < nq:
                qp[s] += dl
                qm[s] -= dl
            else:
                tp, tm = t[k] + dl, t[k] - dl
            (vp, gp, hp), (vm, gm, hm) = f(qp, tp), f(qm, tm)
            g0, g1, g2 = (dq[k, s], gp[s], gm[s]) if s < nq else (dt[k], hp, hm)
            d2[k, s] = abs(vp - 2.0 * L[k] + vm) / dl ** 2
            d3[k, s] = abs(g1 - 2.0 * g0 + g2) / dl ** 2
    d.update(L=L, dq=dq, dt=dt, d2=d2, d3=d3, nq=nq,
             chain=chain_coordinates(model, [m[0] for m in markers]))
    return d


@functools.lru_cache(maxsize=None)
def _evaluated(case, fd):
    """Everything the GPU tests of one (case, scheme) read, computed once:
    with the goal f, its terms, grad f (twice), g, J and the structure; the
    same study without the goal."""
    r = _restated(case)
    x = r["x"]
    st = _study(case, fd)
    nlp = _nlp(case, st)
    d = {"st": st, "h": st.solver.fd_step}
    assert nlp.n == r["n"]
    d["f"], d["terms"], d["grad"] = nlp.eval_f(x), nlp.objective_terms(x), nlp.eval_grad_f(x)
    d["f2"], d["grad2"] = nlp.eval_f(x), nlp.eval_grad_f(x)
    d["g"], d["J"] = nlp.eval_g_jac_g(x)
    d["ir"], d["jc"] = nlp.jac_structure()
    nlp.close()
    st0 = _study(case, fd, goal=False)
    nlp0 = _nlp(case, st0)
    assert nlp0.n == r["n"]
    d["f0"], d["grad0"] = nlp0.eval_f(x), nlp0.eval_grad_f(x)
    d["terms0"] = nlp0.objective_terms(x) if st0.problem.goals else np.zeros(0)
    d["g0"], d["J0"] = nlp0.eval_g_jac_g(x)
    d["ir0"], d["jc0"] = nlp0.jac_structure()
    nlp0.close()
    return d


# ---- CPU --------------------------------------------------------------------

def test_restatement_against_closed_forms():
    """The example's two origin markers: m0 = (cos q0, sin q0, 0), m1 = m0 +
    (cos(q0 + q1), sin(q0 + q1), 0); the integrand with weights 100 and 10
    written out by hand; the analytic gradient (coordinates and time) against
    a sixth-order central difference of the restatement."""
    st = configs.double_pendulum_marker_tracking(2)
    rep = st.problem.create_rep()
    goal, markers = tracked_markers(st, rep)
    assert [(m[0], m[2]) for m in markers] == [("b0", 100.0), ("b1", 10.0)]
    model, ms = st.problem.model, rep.struct.model
    f = lambda q, t: integrand(model, ms, markers, np.asarray(q, float), t)
    for q, t in (([0.3, -0.8], 0.1234), ([-1.1, 0.4], 0.5), ([0.0, 1.3], 0.8321)):
        r0, r1 = t * 0.5 * math.pi, t * 0.25 * math.pi     # the data, splined (times away from the ends' natural end conditions)
        ref0 = np.array([math.cos(r0), math.sin(r0), 0.0])
        ref1 = ref0 + np.array([math.cos(r0 + r1), math.sin(r0 + r1), 0.0])
        got0 = [table_value(ms, markers[0][3], c, t)[0] for c in markers[0][4]]
        got1 = [table_value(ms, markers[1][3], c, t)[0] for c in markers[1][4]]
        assert np.abs(np.array(got0) - ref0).max() < 1e-9 and np.abs(np.array(got1) - ref1).max() < 1e-9
        m0 = np.array([math.cos(q[0]), math.sin(q[0]), 0.0])
        m1 = m0 + np.array([math.cos(q[0] + q[1]), math.sin(q[0] + q[1]), 0.0])
        want = 100.0 * ((m0 - got0) @ (m0 - got0)) + 10.0 * ((m1 - got1) @ (m1 - got1))
        L, dq, dt = f(q, t)
        assert L == pytest.approx(want, rel=1e-13)
        e = 1e-2

        def diff(fun):   # sixth-order central difference
            return (45.0 * (fun(e) - fun(-e)) - 9.0 * (fun(2 * e) - fun(-2 * e)) + (fun(3 * e) - fun(-3 * e))) / (60 * e)
        for s in range(2):
            num = diff(lambda a: f([q[j] + (a if j == s else 0.0) for j in range(2)], t)[0])
            assert dq[s] == pytest.approx(num, rel=1e-8, abs=1e-8)
        assert dt == pytest.approx(diff(lambda a: f(q, t + a)[0]), rel=1e-8, abs=1e-8)
    # at a data row on the reference motion the integrand vanishes
    t = 0.37
    L, dq, dt = f([t * 0.5 * math.pi, t * 0.25 * math.pi], t)
    assert L < 1e-20 and np.abs(dq).max() < 1e-9


def test_lowering_terms_table_and_weights():
    st = configs.double_pendulum_marker_tracking(4)
    rep = st.problem.create_rep()
    p = rep.struct
    assert p.ngoals == 1 and p.nterms == 8
    G = p.goals[0]
    bi, ti = rep.compiled.body_index, rep.compiled.table_index["markers_reference"]
    assert (G.kind, G.table, G.term_begin, G.term_count, G.weight) == (abi.MH_GOAL_MARKER_TRACKING, ti, 0, 8, 1.0)
    assert abi.MH_GOAL_MARKER_TRACKING == 7
    assert [p.goal_index[k] for k in range(8)] == [bi["b0"]] * 4 + [bi["b1"]] * 4
    assert [p.goal_column[k] for k in range(8)] == [0, 1, 2, -1, 3, 4, 5, -1]
    assert [p.goal_weight[k] for k in range(8)] == [0, 0, 0, 100.0, 0, 0, 0, 10.0]
    assert rep.compiled.table_columns["markers_reference"] == [
        f"/markerset/m{i}_{c}" for i in (0, 1) for c in (1, 2, 3)]
    T = p.model.tables[ti]
    assert (T.ncol, T.degree, T.nseg) == (6, 5, 99)
    ref = st.problem.goals[0].markers_reference
    assert list(ref.times[[0, 1, -1]]) == pytest.approx([0.0, 0.01, 0.99], abs=1e-12) and len(ref.times) == 100
    # the table interpolates the rows, built as the state-tracking table is
    for r in (0, 17, 99):
        for c in range(6):
            assert table_value(p.model, ti, c, ref.times[r])[0] == pytest.approx(
                ref.positions[r, c // 3, c % 3], abs=1e-12)
    # the gait variant: bodies, the off-origin locations, the ground marker
    st = configs.gait10dof18musc_marker_track_few(3)
    rep = st.problem.create_rep()
    p, bi = rep.struct, rep.compiled.body_index
    G = p.goals[0]
    assert (G.kind, G.term_count) == (abi.MH_GOAL_MARKER_TRACKING, 20) and p.goals[1].kind == abi.MH_GOAL_CONTROL
    assert [p.goal_index[4 * m] for m in range(5)] == [bi["pelvis"], bi["femur_r"], bi["tibia_l"], bi["calcn_r"], -1]
    assert [p.goal_weight[8 + k] for k in range(4)] == [0.03, -0.2, -0.05, 1.0]
    assert [p.goal_weight[16 + k] for k in range(4)] == [0.3, 0.1, -0.2, 1.0]
    assert (st.problem.time_initial.lower, st.problem.time_final.upper) == (0.0, 2.5)
    # the headline variant
    st = configs.gait10dof18musc_marker_track(2)
    p = st.problem.create_rep().struct
    assert p.goals[0].term_count == 4 * len(configs.GAIT_MARKERS) and len(configs.GAIT_MARKERS) >= 12
    assert [g.name for g in st.problem.goals] == ["marker_tracking", "control_effort"]


def _pendulum_with(labels, allow=False, weights=None):
    """The example with another reference: labels (three constant columns each)."""
    st = configs.double_pendulum_marker_tracking(2)
    m = st.problem.model
    times = np.linspace(0.0, 1.0, 12)
    pos = np.zeros((12, len(labels), 3))
    for i in range(len(labels)):
        pos[:, i, :] = [0.5 + i, 0.25 * i, 0.0]
    ref = MarkersReference("markers_reference", times, list(labels), pos, dict(weights or {}))
    if len(set(labels)) == len(labels):
        m.add_table(ref.flatten())
    st.problem.goals = [MocoMarkerTrackingGoal("marker_tracking", 1.0, ref, allow_unused_references=allow)]
    return st


def test_lowering_reports_the_reference_errors(tmp_path):
    """MocoMarkerTrackingGoal.cpp:39-67, by the Python lowering and by the C++
    builder: redundant labels, an unknown marker, allow_unused_references
    dropping a column, and a label that is a marker-set name."""
    bad = [(_pendulum_with(["/markerset/m0", "m1", "/markerset/m0"]), "Label '/markerset/m0' appears more than once."),
           (_pendulum_with(["/markerset/m0", "m7"]), "Marker 'm7' unrecognized by the specified model."),
           (_pendulum_with(["/markerset/m0"], weights={"/markerset/m0": -1.0}), "negative weight")]
    for st, msg in bad:
        with pytest.raises(ValueError) as ei:
            st.problem.create_rep()
        assert msg in str(ei.value)
        desc = tmp_path / "bad.mhdesc"
        write_description(st, str(desc))
        r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "bad.tape")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (msg, r.stderr)
    with pytest.raises(ValueError, match="appears more than once"):
        bad[0][0].problem.goals[0].markers_reference.flatten()
    # an unused reference is dropped: its columns stay in the table, no term reads them;
    # "m1" is found by its name in the marker set; weights go by reference index
    st = _pendulum_with(["m7", "m1", "/markerset/m0"], allow=True, weights={"m1": 3.0, "m7": 5.0})
    rep = st.problem.create_rep()
    p, bi = rep.struct, rep.compiled.body_index
    assert p.goals[0].term_count == 8
    assert [p.goal_index[k] for k in range(8)] == [bi["b1"]] * 4 + [bi["b0"]] * 4
    assert [p.goal_column[k] for k in range(8)] == [3, 4, 5, -1, 6, 7, 8, -1]
    assert [p.goal_weight[3], p.goal_weight[7]] == [3.0, 1.0]
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    write_tape(rep, st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()
    # a goal without its table in the model
    st = _pendulum_with(["m0"])
    del st.problem.model.tables["markers_reference"]
    with pytest.raises(ValueError, match="reference table markers_reference not in model"):
        st.problem.create_rep()


@pytest.mark.parametrize("name", ["pendulum", "pendulum_trapezoidal", "gait_few", "gait"])
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    problem.py (as tests/test_builder.py compares)."""
    st = {"pendulum": lambda: configs.double_pendulum_marker_tracking(4),
          "pendulum_trapezoidal": lambda: configs.double_pendulum_marker_tracking(3, "trapezoidal", "forward"),
          "gait_few": lambda: configs.gait10dof18musc_marker_track_few(3),
          "gait": lambda: configs.gait10dof18musc_marker_track(3)}[name]()
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


def _info(st, mutate=None):
    info = abi.mh_nlp_info()
    rep, opts = st.problem.create_rep(), st.solver.options()
    if mutate:
        mutate(rep.struct)
    rc = abi.load_mocohip().mh_get_nlp_info_for(C.byref(rep.struct), C.byref(opts), C.byref(info))
    return rc, info, rep   # rep keeps the arrays alive


def _bad_problems():
    """(study, mutation of its mh_problem, message, error code)."""
    pend = lambda: configs.double_pendulum_marker_tracking(2)
    cols = np.zeros(64, np.int32)

    def seti(field, k, v):
        def f(p):
            getattr(p, field)[k] = v
        return f

    def setg(**kw):
        def f(p):
            for k, v in kw.items():
                setattr(p.goals[0], k, v)
        return f

    def prescribe(p):   # every coordinate from column 0 of the model's first table
        p.prescribed_kinematics = 1
        p.kinematics_table = 0
        p.kinematics_column = abi.iptr(cols)
    return [
        (pend, seti("goal_index", 0, 2), "index 2 out of range", abi.MH_ERR_INVALID),
        (pend, seti("goal_index", 4, -2), "index -2 out of range", abi.MH_ERR_INVALID),
        (pend, seti("goal_index", 5, 0), "a marker's terms name different bodies", abi.MH_ERR_INVALID),
        (pend, setg(table=1), "bad table", abi.MH_ERR_INVALID),
        (pend, setg(table=-1), "bad table", abi.MH_ERR_INVALID),
        (pend, seti("goal_column", 1, 6), "column out of range", abi.MH_ERR_INVALID),
        (pend, seti("goal_column", 6, -1), "column out of range", abi.MH_ERR_INVALID),
        (pend, setg(term_count=7), "bad terms", abi.MH_ERR_INVALID),
        (pend, setg(term_count=12), "bad terms", abi.MH_ERR_INVALID),
        (pend, seti("goal_weight", 3, -100.0), "negative marker weight", abi.MH_ERR_INVALID),
        (pend, setg(kind=8), "unknown kind 8", abi.MH_ERR_INVALID),
        (pend, setg(kind=6), "unknown kind 6", abi.MH_ERR_INVALID),
        (lambda: configs.gait10dof18musc_marker_track_few(2, dynamics="implicit"), prescribe, "marker goal needs coordinate states",
         abi.MH_ERR_UNSUPPORTED),
    ]


def test_layout_query_accepts_the_new_problems_and_refuses_what_create_refuses():
    """mh_get_nlp_info_for (host only): the goal changes no layout count, and
    validate_and_layout's refusals come with their messages and codes."""
    lib = abi.load_mocohip()
    for make in (lambda: configs.double_pendulum_marker_tracking(3),
                 lambda: configs.gait10dof18musc_marker_track_few(3),
                 lambda: configs.gait10dof18musc_marker_track(4)):
        st, st0 = make(), make()
        st0.problem.goals = [g for g in st0.problem.goals if not isinstance(g, MocoMarkerTrackingGoal)]
        (rc, a, _), (rc0, b, _) = _info(st), _info(st0)
        assert rc == 0 and rc0 == 0, lib.mh_last_error().decode()
        assert (a.n, a.m, a.nnz_jac_g, a.num_grid_points) == (b.n, b.m, b.nnz_jac_g, b.num_grid_points)
    for make, mutate, msg, code in _bad_problems():
        rc, _, _ = _info(make(), mutate)
        assert rc == code and msg in lib.mh_last_error().decode(), (msg, rc, lib.mh_last_error().decode())
    # nq > 64 is refused like the final-marker goal's: a 65-link pendulum
    m = configs.n_link_pendulum(65)
    from mocohip.model import Marker
    from mocohip.problem import MocoProblem
    from mocohip.solver import MocoHipSolver, MocoStudy
    m.add_marker(Marker("tip", "b64", (0.0, 0.0, 0.0)))
    ref = MarkersReference("markers_reference", np.linspace(0, 1, 8), ["tip"], np.zeros((8, 1, 3)))
    m.add_table(ref.flatten())
    p = MocoProblem(m)
    p.set_time_bounds(0, 1.0)
    p.add_goal(MocoMarkerTrackingGoal("marker_tracking", 1.0, ref))
    rc, _, _ = _info(MocoStudy(p, MocoHipSolver(num_mesh_intervals=2)))
    assert rc == abi.MH_ERR_UNSUPPORTED and "marker goal needs coordinate states" in lib.mh_last_error().decode()


def test_limited_memory_history_option():
    """optim_ipopt_limited_memory_max_history maps to Ipopt's
    limited_memory_max_history: absent at -1 (Ipopt's default, 6), carried
    into the interior-point restatement's options, negative values refused;
    the example's config keeps 100 pairs, every other config the default."""
    from mocohip.ipm import IpmOptions
    from mocohip.solver import MocoHipSolver
    s = MocoHipSolver()
    assert s.optim_ipopt_limited_memory_max_history == -1
    assert "limited_memory_max_history" not in s.ipopt_options()
    assert IpmOptions.from_ipopt(s.ipopt_options()).limited_memory_max_history == 6
    s.optim_ipopt_limited_memory_max_history = 30
    assert s.ipopt_options()["limited_memory_max_history"] == 30
    assert IpmOptions.from_ipopt(s.ipopt_options()).limited_memory_max_history == 30
    s.optim_ipopt_limited_memory_max_history = 0
    assert s.ipopt_options()["limited_memory_max_history"] == 0
    s.optim_ipopt_limited_memory_max_history = -2
    with pytest.raises(ValueError, match="optim_ipopt_limited_memory_max_history"):
        s.ipopt_options()
    assert configs.double_pendulum_marker_tracking(2).solver.ipopt_options()["limited_memory_max_history"] == 100
    assert "limited_memory_max_history" not in configs.gait10dof18musc_marker_track_few(2).solver.ipopt_options()


# ---- GPU --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_objective_against_the_restatement(case, fd):
    """mh_eval_f and the goal's entry of mh_eval_objective_terms: weight *
    duration * sum_k quad_k L_k with the quadrature and the time map of the
    layout; the other goals' terms are those of the study without the goal."""
    r, d = _restated(case), _evaluated(case, fd)
    x, gi = r["x"], r["gi"]
    want = r["goal"].weight * (x[1] - x[0]) * float(r["quad"] @ r["L"])
    got = d["terms"][gi]
    print(f"{case} {fd}: term {got:.17g} restated {want:.17g} |diff| {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-10 * (abs(want) + 1.0)
    assert abs((d["f"] - d["f0"]) - want) <= 1e-10 * (abs(want) + 1.0) + 8 * EPS * abs(d["f0"])
    assert np.array_equal(np.delete(d["terms"], gi), d["terms0"])
    assert want > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_gradient_against_the_restatement(case, fd):
    """mh_eval_grad_f minus the goal-free study's, against the analytic
    gradient: the coordinate entries weight * duration * quad_k dL/dq_s and the
    t0 / tf entries (the integrand's time derivative through the seeds 1 - g
    and g, and -+ weight * sum_k quad_k L_k).  Tolerance per quotient: the
    value error over h plus the scheme's truncation (h / 2 |L''| or h^2 / 6
    |L'''|, from second differences of the restatement, doubled), as in
    test_frame_distance's test_rows_and_jacobian_against_the_restatement."""
    r, d = _restated(case), _evaluated(case, fd)
    x, G, NS, nq, h = r["x"], r["G"], r["NS"], r["nq"], d["h"]
    W, dur, quad, g = r["goal"].weight, x[1] - x[0], r["quad"], r["grid"]
    diff = d["grad"] - d["grad0"]
    want_term = W * dur * float(quad @ r["L"])
    rel = abs(d["terms"][r["gi"]] - want_term) / (abs(want_term) + 1.0)   # measured value error, <= 1e-10
    dv = rel * (np.abs(r["L"]) + 1.0) + 64 * EPS * (np.abs(r["L"]).max() + 1.0)
    trunc = 2.0 * (h * h / 6.0 * r["d3"] if fd == "central" else h / 2.0 * r["d2"])   # [G, nq + 1]
    worst = 0.0
    for k in range(G):
        for s in r["chain"]:
            scale = W * dur * quad[k]
            want = scale * r["dq"][k, s]
            tol = scale * (1e-8 * abs(r["dq"][k, s]) + 8 * dv[k] / h + trunc[k, s])
            got = diff[2 + k * NS + s]
            worst = max(worst, abs(got - want) / tol)
            assert abs(got - want) <= tol, (k, s, got, want, tol)
    acc = float(quad @ r["L"])
    for c, seed in ((0, 1.0 - g), (1, g)):
        want = W * dur * float((quad * seed) @ r["dt"]) + (-W if c == 0 else W) * acc
        tol = W * dur * float((quad * seed) @ (1e-8 * np.abs(r["dt"]) + 8 * dv / h + trunc[:, nq])) \
            + 1e-10 * (W * abs(acc) + 1.0) + 64 * EPS * abs(d["grad0"][c])
        worst = max(worst, abs(diff[c] - want) / tol)
        assert abs(diff[c] - want) <= tol, (c, diff[c], want, tol)
    print(f"{case} {fd}: worst |grad f - ref| / tol = {worst:.3e}")
    assert np.abs(diff).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_exact_zeros_and_nothing_else_moves(case, fd):
    """The goal reads t and the chain coordinates only: every other grad f
    entry -- speeds, auxiliary states, controls, derivatives, multipliers,
    coordinates on no tracked chain (the gait's ankle_angle_l and lumbar_extension) -- has the
    bits of the study without the goal; so have g, the Jacobian and the other
    goals' terms.  The same iterate twice gives the same bits."""
    r, d = _restated(case), _evaluated(case, fd)
    touched = {0, 1} | {2 + k * r["NS"] + s for k in range(r["G"]) for s in r["chain"]}
    same = np.array([i not in touched for i in range(r["n"])])
    assert np.array_equal(d["grad"][same], d["grad0"][same], equal_nan=True)
    if case.startswith("gait"):
        assert len(r["chain"]) == r["nq"] - 2   # ankle_angle_l and lumbar_extension drive no tracked marker
        assert np.abs(d["grad0"][same]).max() > 0.0
    assert np.array_equal(d["g"], d["g0"], equal_nan=True) and np.array_equal(d["J"], d["J0"], equal_nan=True)
    assert np.array_equal(d["ir"], d["ir0"]) and np.array_equal(d["jc"], d["jc0"])
    assert np.array_equal(np.delete(d["terms"], r["gi"]), d["terms0"])
    assert d["f"] == d["f2"] and np.array_equal(d["grad"], d["grad2"], equal_nan=True)
    assert np.isfinite(d["grad"]).all() and math.isfinite(d["f"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pendulum_hs_3", "gait_generated"])
def test_shards_sum_to_the_whole(case):
    """mh_eval_f_partial / mh_eval_grad_f_partial over 2 shards: the f
    partials sum to f within 8 eps sum |partial|; a grad f entry of a grid
    point inside one shard (not a mesh point two shards share) is that
    shard's partial entry, bit for bit, and 0 in the other; the shared mesh
    point's and the t0 / tf entries sum within the same bound."""
    fd = "central" if case.startswith("pendulum") else "forward"
    r, d = _restated(case), _evaluated(case, fd)
    x, G, NS, n = r["x"], r["G"], r["NS"], r["n"]
    st = _study(case, fd)
    N = st.solver.num_mesh_intervals
    step = (G - 1) // N
    cut = 1
    parts = []
    for a, b in ((0, cut), (cut, N)):
        sh = _nlp(case, st, (a, b))
        parts.append((sh.eval_f_partial(x), sh.eval_grad_f_partial(x)))
        sh.close()
    fsum = parts[0][0] + parts[1][0]
    assert abs(fsum - d["f"]) <= 8 * EPS * (abs(parts[0][0]) + abs(parts[1][0]))
    assert parts[0][0] != 0.0 and parts[1][0] != 0.0
    kcut = cut * step
    for s in r["chain"]:
        for k in range(G):
            i = 2 + k * NS + s
            if k < kcut:
                assert parts[0][1][i] == d["grad"][i] and parts[1][1][i] == 0.0, (k, s)
            elif k > kcut:
                assert parts[1][1][i] == d["grad"][i] and parts[0][1][i] == 0.0, (k, s)
    gsum = parts[0][1] + parts[1][1]
    bound = 8 * EPS * (np.abs(parts[0][1]) + np.abs(parts[1][1])) + 1e-12 * np.abs(d["grad"])
    assert (np.abs(gsum - d["grad"]) <= bound).all()


@pytest.mark.gpu
def test_refusals():
    """mh_create refuses what the layout query refuses, before device work."""
    from mocohip.solver import HipNLP
    for make, mutate, msg, _ in _bad_problems():
        st = make()
        rep = st.problem.create_rep()
        mutate(rep.struct)
        with pytest.raises(RuntimeError, match=msg.replace("(", r"\(")):
            HipNLP(rep, st.solver.options())


@pytest.mark.gpu
def test_reference_example_solved_on_the_hip_path():
    """exampleMarkerTracking.cpp through MocoStudy.solve from the bounds
    guess, N = 50: success, and the RMS over the mesh points of (q0, q1)
    against t pi / 2, t pi / 4 is at most 1 % of the bounds guess's RMS (the
    motion is feasible: the gravity torques stay within the +-40 control
    bounds).  Measured: Solve_Succeeded after 347 iterations, RMS 1.507e-5
    (guess 0.72), so the assertion is 10 x that.  The config keeps 100
    limited-memory pairs where the example uses the exact Hessian; with
    Ipopt's default of 6 no finite-difference scheme converges within 3000
    iterations."""
    from mocohip.solver import HipNLP
    st = configs.double_pendulum_marker_tracking()
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    x0 = nlp.initial_guess_from_bounds()
    G, NS = nlp.G, nlp.NS
    nlp.close()

    def rms(t, q0, q1):
        return math.sqrt(np.mean(np.concatenate([(q0 - t * math.pi / 2) ** 2, (q1 - t * math.pi / 4) ** 2])))
    S0 = x0[2:2 + NS * G].reshape(G, NS)[::2]
    t0 = np.linspace(x0[0], x0[1], len(S0))
    rms0 = rms(t0, S0[:, 0], S0[:, 1])
    sol = st.solve()
    assert sol.metadata["success"] == "true", sol.metadata
    t = sol.time[::2]
    got = rms(t, sol.get_state("/jointset/j0/q0/value")[::2], sol.get_state("/jointset/j1/q1/value")[::2])
    print(f"double_pendulum_marker_tracking N=50: {sol.metadata['num_iterations']} iterations, "
          f"RMS {got:.3e} (guess {rms0:.3e}), status {sol.metadata.get('status')}")
    assert got <= 0.01 * rms0
    assert got <= 1.5e-4   # 10 x the measured 1.507e-5
