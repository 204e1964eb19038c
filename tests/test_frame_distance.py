"""MocoFrameDistanceConstraint as a device path constraint
(MocoFrameDistanceConstraint.{h,cpp}; include/mocohip.h MH_PATH_FRAME_DISTANCE*).

The checker of the new rows is a NumPy restatement of the forward kinematics
over the Python Model (parent pose x joint frames x axis functions, float64)
with the three projections and its analytic gradient -- the oracle does not
know these kinds.

CPU: the restatement against closed forms, the lowering (Python and the C++
builder, byte-identical tapes; every reference check with its message) and the
host-only layout query.  GPU: the parity matrix (structure, g, Jacobian,
exact zeros), the Jacobian bit for bit from mh_eval_path's values, nothing
else moving, shards, refusals, and the reference's own test problem solved."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.problem import MocoFrameDistanceConstraint, MocoFrameDistanceConstraintPair
from mocohip.splines import SimmSpline
from mocohip.tape import write_tape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_BUILD = os.path.join(ROOT, "opensim-moco_amd", "csrc", "build", "mh_build")
EPS = np.finfo(float).eps


# ---- the restatement --------------------------------------------------------

def _axis_rot(a, t):
    """Rotation by t about the unit axis a (Rodrigues)."""
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], float)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def _fn(f, q, qidx):
    """Value and derivative of a coordinate function; the coordinate's index."""
    if f.kind == abi.MH_FN_CONSTANT:
        return f.a, 0.0, -1
    s = qidx[f.coord]
    if f.kind == abi.MH_FN_LINEAR:
        return f.scale * (f.a * q[s] + f.b), f.scale * f.a, s
    sp = SimmSpline(f.x, f.y)
    return f.scale * sp(q[s]), f.scale * sp(q[s], 1), s


def forward_kinematics(model, q):
    """body -> (R, p, motions): the pose in ground at coordinates q, and for
    every coordinate-driven axis on the body's ancestor chain (coordinate,
    d value / d q, rotation?, axis or direction in ground, pivot)."""
    from mocohip.model import body_fixed_xyz
    qidx = model.coordinate_index()
    pose = {"ground": (np.eye(3), np.zeros(3), [])}
    for j in model.tree_order():
        Rp, pp, mot = pose[j.parent]
        mot = list(mot)
        RGF = Rp @ body_fixed_xyz(j.orient_in_parent)
        pGF = pp + Rp @ np.asarray(j.loc_in_parent, float)
        pFM = np.zeros(3)
        for ax in j.axes:
            if ax.type != abi.MH_AXIS_TRANSLATION:
                continue
            d = np.asarray(ax.dir, float) / np.linalg.norm(ax.dir)
            v, dv, s = _fn(ax.func, q, qidx)
            pFM = pFM + v * d
            if s >= 0:
                mot.append((s, dv, False, RGF @ d, None))
        oM = pGF + RGF @ pFM
        Rcur = np.eye(3)
        for ax in j.axes:
            if ax.type != abi.MH_AXIS_ROTATION:
                continue
            d = np.asarray(ax.dir, float) / np.linalg.norm(ax.dir)
            v, dv, s = _fn(ax.func, q, qidx)
            if s >= 0:
                mot.append((s, dv, True, RGF @ Rcur @ d, oM))
            Rcur = Rcur @ _axis_rot(d, v)
        Rb = RGF @ Rcur @ body_fixed_xyz(j.orient_in_child).T
        pose[j.child] = (Rb, oM - Rb @ np.asarray(j.loc_in_child, float), mot)
    return pose


def station(model, pose, body, loc, nq):
    """Position in ground of the point loc of body, and its gradient [3, nq]."""
    R, p, mot = pose[body]
    P = p + R @ np.asarray(loc, float)
    dP = np.zeros((3, nq))
    for s, dv, rot, a, pivot in mot:
        dP[:, s] += dv * (np.cross(a, P - pivot) if rot else a)
    return P, dP


def frame_distance(model, q, frame1, frame2, projection="none", vector=None):
    """MocoFrameDistanceConstraint's error for one pair at coordinates q, and
    its gradient along the coordinates."""
    nq = len(q)
    pose = forward_kinematics(model, q)
    (b1, l1), (b2, l2) = model.find_frame(frame1), model.find_frame(frame2)
    P1, dP1 = station(model, pose, b1, l1, nq)
    P2, dP2 = station(model, pose, b2, l2, nq)
    r, dr = P2 - P1, dP2 - dP1
    if projection == "none":
        e, de = r, dr
    else:
        n = np.asarray(vector, float) / np.linalg.norm(vector)
        e, de = (r @ n) * n, np.outer(n, n @ dr)
        if projection == "plane":
            e, de = r - e, dr - de
    return float(e @ e), 2.0 * (e @ de)


def chain_coordinates(model, frames):
    """Coordinates on the ancestor chain of one of the frames' bodies."""
    qidx = model.coordinate_index()
    parent = {j.child: j for j in model.joints}
    out = set()
    for fr in frames:
        b = model.find_frame(fr)[0]
        while b != "ground":
            out.update(qidx[c.name] for c in parent[b].coordinates)
            b = parent[b].parent
    return sorted(out)


# ---- the studies ------------------------------------------------------------

def _pendulum_pair(n, scheme):
    st = configs.double_pendulum(n, scheme=scheme)
    c = st.problem.add_path_constraint(MocoFrameDistanceConstraint())
    c.add_frame_pair("/ground", "/bodyset/b1", 0.1, math.inf)
    return st


CASES = {
    "pendulum_hs": (lambda: _pendulum_pair(3, "hermite-simpson"), None),
    "pendulum_trapezoidal": (lambda: _pendulum_pair(3, "trapezoidal"), None),
    "gimbal_explicit": (lambda: configs.gimbal_frame_distance(2, dynamics="explicit"), None),
    "gimbal_implicit": (lambda: configs.gimbal_frame_distance(2, dynamics="implicit"), None),
}
for _proj in ("none", "vector", "plane"):
    for _be in ("generated", "generic"):
        CASES[f"gait_{_proj}_{_be}"] = (functools.partial(configs.gait10dof18musc_feet_apart, 2, _proj), _be)
FDS = ("forward", "backward", "central")
MATRIX = [(c, fd) for c in CASES for fd in FDS]


def _study(case, fd, constraint=True, detection="none"):
    st = CASES[case][0]()
    st.solver.optim_finite_difference_scheme = fd
    st.solver.optim_sparsity_detection = detection
    if not constraint:
        st.problem.path_constraints = [pc for pc in st.problem.path_constraints
                                       if not isinstance(pc, MocoFrameDistanceConstraint)]
    return st


def _nlp(case, st):
    from mocohip.solver import HipNLP
    generic = CASES[case][1] == "generic"
    if generic:
        os.environ["MOCOHIP_BACKEND"] = "generic"
    try:
        nlp = HipNLP(st.problem.create_rep(), st.solver.options())
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


def _pairs(st):
    out = []
    for pc in st.problem.path_constraints:
        if isinstance(pc, MocoFrameDistanceConstraint):
            out += [(fp, pc.projection, pc.projection_vector) for fp in pc.frame_pairs]
    return out


def _new_rows(nlp, st):
    """Rows of g that are frame-distance rows: [mesh point][pair], found by
    their bounds [minimum^2, maximum^2] (every other row's lower bound is 0
    or -inf)."""
    gl, gu = nlp.bounds()[2:]
    pairs = _pairs(st)
    rows = [r for r in range(nlp.m) if any(gl[r] == fp.minimum_distance ** 2 and gu[r] == fp.maximum_distance ** 2
                                           for fp, _, _ in pairs)]
    N = st.solver.num_mesh_intervals
    assert len(rows) == len(pairs) * (N + 1)
    return np.asarray(rows).reshape(N + 1, len(pairs))


@functools.lru_cache(maxsize=None)
def _evaluated(case, fd):
    """Everything the GPU tests of one case read, computed once: the
    constrained context's structure, g and J at a random in-bounds iterate
    (twice), the same problem's without the constraint, the detected
    structure, and mh_eval_path's values at the base and perturbed rows."""
    st = _study(case, fd)
    nlp = _nlp(case, st)
    d = {"st": st, "n": nlp.n, "m": nlp.m, "G": nlp.G, "NS": nlp.NS, "NC": nlp.NC, "NI": nlp.NI, "NQ": nlp.NQ}
    x = _iterate(nlp, case.startswith("gait"))
    d["x"] = x
    d["ir"], d["jc"] = nlp.jac_structure()
    d["rows"] = _new_rows(nlp, st)
    d["g"], d["J"] = nlp.eval_g_jac_g(x)
    d["g_alone"], d["J_alone"] = nlp.eval_g(x), nlp.eval_jac_g(x)
    d["g2"], d["J2"] = nlp.eval_g_jac_g(x)
    # the device's own lanes: base row, then coordinate s at +h and at -h
    step = 2 if st.solver.transcription_scheme == "hermite-simpson" else 1
    h = st.solver.fd_step
    pin = nlp.point_inputs(x)[::step]
    base = np.concatenate([np.zeros((len(pin), 1)), pin], 1)
    rows = [base]
    for sign in (1.0, -1.0):
        for s in range(nlp.NQ):
            r = base.copy()
            r[:, 1 + s] = base[:, 1 + s] + h if sign > 0 else base[:, 1 + s] - h
            rows.append(r)
    d["probe"] = nlp.eval_path(np.concatenate(rows)).reshape(1 + 2 * nlp.NQ, len(pin), -1)
    nlp.close()
    st0 = _study(case, fd, constraint=False)
    nlp0 = _nlp(case, st0)
    assert nlp0.n == d["n"]
    d["g0"], d["J0"] = nlp0.eval_g_jac_g(x)
    d["ir0"], d["jc0"] = nlp0.jac_structure()
    nlp0.close()
    std = _study(case, fd, detection="random")
    nlpd = _nlp(case, std)
    d["ird"], d["jcd"] = nlpd.jac_structure()
    d["rowsd"] = _new_rows(nlpd, std)
    nlpd.close()
    return d


# ---- CPU --------------------------------------------------------------------

def test_restatement_against_closed_forms():
    """Two-link pendulum: |b1 origin|^2 = 2 + 2 cos q1 (gradient -2 sin q1
    along q1, 0 along q0); the gimbal's body origin at q = 0 is the ground
    origin; the "vector" and "plane" errors sum to "none"; the analytic
    gradient against a central difference of the restatement itself."""
    m = configs.n_link_pendulum(2)
    for q in ([0.3, -0.8], [-1.1, 0.4], [0.0, 1.3]):
        e, de = frame_distance(m, np.array(q), "/ground", "/bodyset/b1")
        assert e == pytest.approx(2.0 + 2.0 * math.cos(q[1]), rel=1e-14)
        assert de == pytest.approx([0.0, -2.0 * math.sin(q[1])], abs=1e-14)
    gm = configs.gimbal_frame_distance(2).problem.model
    assert frame_distance(gm, np.zeros(3), "/ground", "/bodyset/body")[0] == pytest.approx(0.0, abs=1e-30)
    # the body center (offset frame, 0.5 from the joint) stays 0.5 from (0, 1, 0)
    e, _ = frame_distance(gm, np.array([0.3, -0.5, 0.2]), "/ground", "/bodyset/body/body_center")
    P = station(gm, forward_kinematics(gm, np.array([0.3, -0.5, 0.2])), "body", (-0.5, 0, 0), 3)[0]
    assert np.linalg.norm(P - [0, 1, 0]) == pytest.approx(0.5, rel=1e-14) and e == pytest.approx(P @ P)
    st = configs.gait10dof18musc_feet_apart(2, "plane")
    fm = st.problem.model
    fp, _, vec = _pairs(st)[0]
    q = np.random.default_rng(3).uniform(-0.4, 0.4, len(fm.coordinates()))
    vals = {p: frame_distance(fm, q, fp.frame1_path, fp.frame2_path, p, vec) for p in ("none", "vector", "plane")}
    assert vals["vector"][0] + vals["plane"][0] == pytest.approx(vals["none"][0], rel=1e-13)
    d = 1e-6
    for p, (e, de) in vals.items():
        for s in range(len(q)):
            qp, qm = q.copy(), q.copy()
            qp[s] += d
            qm[s] -= d
            num = (frame_distance(fm, qp, fp.frame1_path, fp.frame2_path, p, vec)[0] -
                   frame_distance(fm, qm, fp.frame1_path, fp.frame2_path, p, vec)[0]) / (2 * d)
            assert de[s] == pytest.approx(num, abs=1e-8), (p, s)
    chain = chain_coordinates(fm, [fp.frame1_path, fp.frame2_path])
    off = [s for s in range(len(q)) if s not in chain]
    assert off and all(vals["none"][1][s] == 0.0 for s in off)   # lumbar: off both chains


def test_lowering_equations_bounds_and_terms():
    st = configs.gimbal_frame_distance(3)
    rep = st.problem.create_rep()
    p = rep.struct
    assert p.npath == 1 and rep.num_path_equations == 1
    e = p.path[0]
    assert (e.kind, e.index, e.table) == (abi.MH_PATH_FRAME_DISTANCE, -1, 0)
    assert (e.g.lower, e.g.upper) == (0.1 * 0.1, math.inf)
    # the marker goal's six terms, then the equation's nine
    assert e.column == 6 and p.nterms == 15
    assert [p.goal_weight[e.column + k] for k in range(9)] == [0.0] * 9
    assert [p.goal_index[e.column + k] for k in range(9)] == [0] * 9
    for proj, kind in (("none", abi.MH_PATH_FRAME_DISTANCE), ("vector", abi.MH_PATH_FRAME_DISTANCE_VECTOR),
                       ("plane", abi.MH_PATH_FRAME_DISTANCE_PLANE)):
        st = configs.gait10dof18musc_feet_apart(2, proj)
        rep = st.problem.create_rep()
        p = rep.struct
        e = p.path[0]
        bi = rep.compiled.body_index
        assert (e.kind, e.index, e.table) == (kind, bi["calcn_r"], bi["calcn_l"])
        assert (e.g.lower, e.g.upper) == (0.1 * 0.1, math.inf)
        assert e.column + 9 == p.nterms
        w = [p.goal_weight[e.column + k] for k in range(9)]
        assert w[:6] == [0.1, 0.02, 0.01, 0.1, 0.02, -0.01]
        if proj == "none":
            assert w[6:] == [0.0, 0.0, 0.0]
        else:
            n = np.array([0.1, 0.2, 1.0])
            assert w[6:] == pytest.approx(n / np.linalg.norm(n), rel=1e-15)
            assert np.linalg.norm(w[6:]) == pytest.approx(1.0, rel=1e-15)
    # a control-bound constraint before it keeps its own table reference
    st = configs.gait10dof18musc(2, control_bounds=True)
    ncb = st.problem.create_rep().struct.npath
    c = st.problem.add_path_constraint(MocoFrameDistanceConstraint())
    c.add_frame_pair("calcn_r", "/ground", 0.0, 2.0)
    p = st.problem.create_rep().struct
    assert p.npath == ncb + 1 and p.path[ncb].kind == abi.MH_PATH_FRAME_DISTANCE
    assert (p.path[ncb].g.lower, p.path[ncb].g.upper, p.path[ncb].table) == (0.0, 4.0, -1)
    assert all(p.path[k].kind == abi.MH_PATH_CONTROL_BOUND for k in range(ncb))


def _bad_studies():
    def make(**kw):
        st = configs.gimbal_frame_distance(2)
        c = st.problem.path_constraints[0]
        fp = c.frame_pairs[0]
        for k, v in kw.items():
            setattr(fp if hasattr(fp, k) else c, k, v)
        return st
    return [
        (make(frame1_path="/bodyset/nobody"), "Could not find frame '/bodyset/nobody'."),
        (make(frame2_path="/ground/nothing"), "Could not find frame '/ground/nothing'."),
        (make(minimum_distance=-0.5), "Expected the minimum distance for this frame pair to non-negative, but it is"),
        (make(minimum_distance=0.0, maximum_distance=-1.0),
         "Expected the maximum distance for this frame pair to non-negative, but it is"),
        (make(minimum_distance=2.0, maximum_distance=1.0),
         "Expected the minimum distance for this frame pair to be less than or equal to the maximum distance"),
        (make(projection="line"), "Expected 'projection' to be 'none', 'vector', or 'plane', but got 'line'."),
        (make(projection="plane"), "Must provide a value for 'projection_vector'."),
    ]


def test_lowering_reports_the_reference_errors(tmp_path):
    """MocoFrameDistanceConstraint.cpp:65-107, by the Python lowering and by
    the C++ builder."""
    for st, msg in _bad_studies():
        with pytest.raises(ValueError) as ei:
            st.problem.create_rep()
        assert msg in str(ei.value)
        desc = tmp_path / "bad.mhdesc"
        write_description(st, str(desc))
        r = subprocess.run([MH_BUILD, str(desc), str(tmp_path / "bad.tape")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (msg, r.stderr)
    st = configs.gimbal_frame_distance(2)
    st.problem.path_constraints.append(MocoFrameDistanceConstraintPair("/ground", "/bodyset/body"))
    with pytest.raises(TypeError, match="unsupported path constraint"):
        st.problem.create_rep()


@pytest.mark.parametrize("name", ["gimbal", "gimbal_implicit", "gait_none", "gait_vector", "gait_plane",
                                  "gait_with_control_bounds"])
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    problem.py (as tests/test_builder.py compares)."""
    if name.startswith("gimbal"):
        st = configs.gimbal_frame_distance(4, dynamics="implicit" if name.endswith("implicit") else "explicit")
    elif name == "gait_with_control_bounds":
        st = configs.gait10dof18musc_feet_apart(3, "vector", control_bounds=True)
    else:
        st = configs.gait10dof18musc_feet_apart(3, name.split("_")[1])
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


def _info(st):
    info = abi.mh_nlp_info()
    rep, opts = st.problem.create_rep(), st.solver.options()
    rc = abi.load_mocohip().mh_get_nlp_info_for(C.byref(rep.struct), C.byref(opts), C.byref(info))
    return rc, info


@pytest.mark.parametrize("case", ["pendulum_hs", "pendulum_trapezoidal", "gimbal_implicit", "gait_none_generated"])
def test_layout_query_adds_one_row_per_pair_and_mesh_point(case):
    """mh_get_nlp_info_for (host only): the same problem minus the constraint,
    plus one row per pair per mesh point, block-dense over t0, tf and the
    mesh point's inputs."""
    st, st0 = _study(case, "forward"), _study(case, "forward", constraint=False)
    (rc, a), (rc0, b) = _info(st), _info(st0)
    assert rc == 0 and rc0 == 0
    N, npair = st.solver.num_mesh_intervals, len(_pairs(st))
    NI = int(a.num_states) + int(a.num_controls) + (len(st.problem.model.coordinates())
                                                    if st.solver.multibody_dynamics_mode == "implicit" else 0)
    assert a.n == b.n
    assert a.m == b.m + npair * (N + 1)
    assert a.nnz_jac_g == b.nnz_jac_g + npair * (N + 1) * (2 + NI)


def test_layout_query_refuses_what_create_refuses():
    """validate_and_layout's checks, through the host-only query: body index,
    term range, bounds, prescribed kinematics, a projection without a vector."""
    lib = abi.load_mocohip()

    def refused(mutate, msg, st=None):
        st = st or configs.gimbal_frame_distance(2)
        rep, opts = st.problem.create_rep(), st.solver.options()
        mutate(rep.struct)
        info = abi.mh_nlp_info()
        assert lib.mh_get_nlp_info_for(C.byref(rep.struct), C.byref(opts), C.byref(info)) != 0
        assert msg in lib.mh_last_error().decode(), lib.mh_last_error().decode()

    def setp(**kw):
        def f(p):
            for k, v in kw.items():
                if k in ("lower", "upper"):
                    setattr(p.path[0].g, k, v)
                else:
                    setattr(p.path[0], k, v)
        return f
    refused(setp(table=1), "frame body out of range")
    refused(setp(index=-2), "frame body out of range")
    refused(setp(column=7), "term range out of range")
    refused(setp(column=-1), "term range out of range")
    refused(setp(lower=-0.01), "negative or inverted distance bounds")
    refused(setp(lower=4.0, upper=1.0), "negative or inverted distance bounds")
    refused(setp(kind=abi.MH_PATH_FRAME_DISTANCE_PLANE), "zero projection vector")
    refused(setp(kind=4), "kind 4")

    cols = np.zeros(64, np.int32)

    def prescribe(p):   # every coordinate from column 0 of the model's first table
        p.prescribed_kinematics = 1
        p.kinematics_table = 0
        p.kinematics_column = abi.iptr(cols)
    refused(prescribe, "frame distance needs coordinate states",
            configs.gait10dof18musc_feet_apart(2, "none", dynamics="implicit"))


# ---- GPU --------------------------------------------------------------------

def _entries(d, rows, ir):
    """Jacobian entries of the frame-distance rows: [(entry, mesh point, pair)]."""
    where = {int(r): (i, e) for i, rr in enumerate(rows) for e, r in enumerate(rr)}
    return [(k, *where[int(r)]) for k, r in enumerate(ir) if int(r) in where]


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_rows_and_jacobian_against_the_restatement(case, fd):
    d = _evaluated(case, fd)
    st, x, G, NS, NQ = d["st"], d["x"], d["G"], d["NS"], d["NQ"]
    model, pairs = st.problem.model, _pairs(st)
    N = st.solver.num_mesh_intervals
    step = (G - 1) // N
    h = st.solver.fd_step
    # structure: block-dense over t0, tf and the mesh point's inputs
    ent = _entries(d, d["rows"], d["ir"])
    assert len(ent) == len(pairs) * (N + 1) * (2 + d["NI"])
    for i in range(N + 1):
        for e in range(len(pairs)):
            cols = sorted(int(d["jc"][k]) for k, ii, ee in ent if (ii, ee) == (i, e))
            assert len(set(cols)) == 2 + d["NI"] and cols[:2] == [0, 1]
            k = i * step
            want = set(range(2 + k * NS, 2 + (k + 1) * NS)) | set(
                range(2 + NS * G + k * d["NC"], 2 + NS * G + (k + 1) * d["NC"]))
            assert want <= set(cols)
    # with detection: only the chain coordinates of the mesh point
    entd = _entries(d, d["rowsd"], d["ird"])
    for e, (fp, _, _) in enumerate(pairs):
        chain = chain_coordinates(model, [fp.frame1_path, fp.frame2_path])
        for i in range(N + 1):
            cols = sorted(int(d["jcd"][k]) for k, ii, ee in entd if (ii, ee) == (i, e))
            # (a chain coordinate the distance does not depend on, like the
            # pendulum's q0 for |b1 origin|, is rightly not detected)
            assert cols and set(cols) <= {2 + i * step * NS + s for s in chain}, (i, e, cols)
    # values
    S = x[2:2 + NS * G].reshape(G, NS)
    ref = np.zeros((N + 1, len(pairs)))
    grad = np.zeros((N + 1, len(pairs), NQ))
    trunc = np.zeros_like(grad)
    dl = 1e-3
    for i in range(N + 1):
        q = S[i * step, :NQ]
        for e, (fp, proj, vec) in enumerate(pairs):
            f = lambda qq: frame_distance(model, qq, fp.frame1_path, fp.frame2_path, proj, vec)
            ref[i, e], grad[i, e] = f(q)
            for s in range(NQ):
                qp, qm = q.copy(), q.copy()
                qp[s] += dl
                qm[s] -= dl
                (vp, gp), (vm, gm) = f(qp), f(qm)
                d2 = abs(vp - 2.0 * ref[i, e] + vm) / dl ** 2           # |f''|
                d3 = abs(gp[s] - 2.0 * grad[i, e, s] + gm[s]) / dl ** 2   # |f'''|
                # the scheme's truncation (h / 2 f'', h^2 / 6 f'''), doubled for
                # the second differences' own error
                trunc[i, e, s] = 2.0 * (h * h / 6.0 * d3 if fd == "central" else h / 2.0 * d2)
    got = d["g"][d["rows"]]
    err = np.abs(got - ref).max()
    print(f"{case} {fd}: max |g - ref| = {err:.3e} (max |ref| {np.abs(ref).max():.3e})")
    assert err <= 1e-10 * (np.abs(ref).max() + 1.0)
    dg = err + 64 * EPS * (np.abs(ref).max() + 1.0)
    worst = 0.0
    for k, i, e in ent:
        c = int(d["jc"][k]) - (2 + i * step * NS)
        chain = chain_coordinates(model, [pairs[e][0].frame1_path, pairs[e][0].frame2_path])
        if 0 <= c < NQ and int(d["jc"][k]) >= 2 and c in chain:
            tol = 1e-8 * abs(grad[i, e, c]) + 8 * dg / h + trunc[i, e, c]
            worst = max(worst, abs(d["J"][k] - grad[i, e, c]) / tol)
            assert abs(d["J"][k] - grad[i, e, c]) <= tol, (i, e, c, d["J"][k], grad[i, e, c], tol)
        else:   # time, a non-coordinate input, a coordinate off both chains
            assert d["J"][k] == 0.0, (i, e, c, d["J"][k])
    print(f"{case} {fd}: worst |J - ref| / tol = {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_jacobian_bit_exact_from_the_path_probe(case, fd):
    """Every new entry is the quotient, formed here, of mh_eval_path's values
    at the base and perturbed probe rows, and every new row the base value."""
    d = _evaluated(case, fd)
    st, G, NS, NQ = d["st"], d["G"], d["NS"], d["NQ"]
    N = st.solver.num_mesh_intervals
    step = (G - 1) // N
    h = st.solver.fd_step
    probe = d["probe"]          # [lane][mesh point][equation]
    rows = d["rows"]
    npc = probe.shape[2]
    off = npc - rows.shape[1]   # the frame-distance equations are the last ones of these studies
    assert np.array_equal(d["g"][rows], probe[0][:, off:])
    for k, i, e in _entries(d, rows, d["ir"]):
        c = int(d["jc"][k]) - (2 + i * step * NS)
        if not (int(d["jc"][k]) >= 2 and 0 <= c < NQ):
            continue
        v0, vp, vm = probe[0, i, off + e], probe[1 + c, i, off + e], probe[1 + NQ + c, i, off + e]
        want = (vp - vm) / (2.0 * h) if fd == "central" else (vp - v0) / h if fd == "forward" else (v0 - vm) / h
        assert d["J"][k] == want, (i, e, c, d["J"][k], want)


@pytest.mark.gpu
@pytest.mark.parametrize("case,fd", MATRIX)
def test_nothing_else_moves(case, fd):
    """Without the new rows and entries, g and J are bit for bit those of a
    context on the same problem without the constraint; the same iterate
    twice (and g, J on their own) gives the same bits."""
    d = _evaluated(case, fd)
    new_rows = set(int(r) for r in d["rows"].ravel())
    keep_g = np.array([r not in new_rows for r in range(d["m"])])
    keep_J = np.array([int(r) not in new_rows for r in d["ir"]])
    assert np.array_equal(d["g"][keep_g], d["g0"], equal_nan=True)
    assert np.array_equal(d["J"][keep_J], d["J0"], equal_nan=True)
    assert np.array_equal(d["jc"][keep_J], d["jc0"])
    assert np.array_equal(d["g"], d["g2"], equal_nan=True) and np.array_equal(d["J"], d["J2"], equal_nan=True)
    assert np.array_equal(d["g"], d["g_alone"], equal_nan=True)
    assert np.array_equal(d["J"], d["J_alone"], equal_nan=True)
    assert np.isfinite(d["g"][d["rows"]]).all()


@pytest.mark.gpu
def test_shards_reassemble_bit_exact():
    """Mesh shards (0,2), (2,5), (5,6) concatenate to the unsharded g and J:
    the last one carries the final mesh point's tail row."""
    from mocohip.solver import HipNLP
    st = configs.gait10dof18musc_feet_apart(6, "none")
    rep = st.problem.create_rep()
    full = HipNLP(rep, st.solver.options())
    x = _iterate(full, True)
    g, J = full.eval_g(x), full.eval_jac_g(x)
    rows = _new_rows(full, st)
    assert int(rows[-1, 0]) > full.m - 1 - 2 * full.NS and np.isfinite(g[rows]).all()
    gs, Js = [], []
    for a, b in [(0, 2), (2, 5), (5, 6)]:
        sh = HipNLP(rep, st.solver.options(a, b))
        gs.append(sh.eval_g(x))
        Js.append(sh.eval_jac_g(x))
        sh.close()
    full.close()
    assert np.array_equal(np.concatenate(gs), g, equal_nan=True)
    assert np.array_equal(np.concatenate(Js), J, equal_nan=True)


@pytest.mark.gpu
def test_refusals():
    """mh_batch_* does not serve these kinds; bad indices and prescribed
    kinematics are refused by mh_create before any device work."""
    from mocohip.solver import HipBatch, HipNLP
    st = configs.gait10dof18musc_feet_apart(2, "none")
    nlps = [HipNLP(st.problem.create_rep(), st.solver.options()) for _ in range(2)]
    try:
        with pytest.raises(RuntimeError, match="frame-distance"):
            HipBatch(nlps)
    finally:
        for n in nlps:
            n.close()
    st = configs.gimbal_frame_distance(2)
    rep = st.problem.create_rep()
    rep.struct.path[0].table = 5
    with pytest.raises(RuntimeError, match="frame body out of range"):
        HipNLP(rep, st.solver.options())
    rep = st.problem.create_rep()
    rep.struct.path[0].column = 1000
    with pytest.raises(RuntimeError, match="term range out of range"):
        HipNLP(rep, st.solver.options())
    rep = st.problem.create_rep()
    rep.struct.prescribed_kinematics = 1
    with pytest.raises(RuntimeError, match="Prescribed kinematics|frame distance needs coordinate states"):
        HipNLP(rep, st.solver.options())


@pytest.mark.gpu
def test_reference_problem_solved_on_the_hip_path():
    """testConstraints.cpp:1591-1658 through MocoStudy.solve: success, and at
    every mesh point of the solution the body origin is at least 0.1 - 1e-3
    (the reference's margin, :1654-1656) from the ground origin, while the
    bounds-derived initial guess comes closer than 0.1: the constraint acts.
    N = 25.  The reserves keep the reference's infinite control bounds.  The
    config solves with forward differences (109 iterations); with the
    reference's default, central, mocohip.ipm ends in Restoration_Failed from
    this guess (N = 25: after 46 iterations at a violation of 8e-6; N = 50,
    100: after 4, a mesh point of the guess sits where the constraint's
    gradient vanishes) -- DESIGN.md."""
    from mocohip.solver import HipNLP
    st = configs.gimbal_frame_distance(25)
    model = st.problem.model
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    x0 = nlp.initial_guess_from_bounds()
    xl, xu = nlp.bounds()[:2]
    G, NS, NC = nlp.G, nlp.NS, nlp.NC
    assert np.isinf(xl[2 + NS * G:2 + (NS + NC) * G]).all() and np.isinf(xu[2 + NS * G:2 + (NS + NC) * G]).all()
    nlp.close()

    def distances(S):
        return np.array([math.sqrt(frame_distance(model, q[:3], "/ground", "/bodyset/body")[0]) for q in S])
    d0 = distances(x0[2:2 + NS * G].reshape(G, NS)[::2])
    assert d0.min() < 0.1
    sol = st.solve()
    assert sol.metadata["success"] == "true", sol.metadata
    q = np.stack([sol.get_state(f"/jointset/gimbal/{n}/value") for n in ("qx", "qy", "qz")], 1)
    d = distances(q[::2])
    print(f"gimbal N=25: {sol.metadata['num_iterations']} iterations, min distance {d.min():.6f} "
          f"(guess {d0.min():.6f})")
    assert d.min() >= 0.1 - 1e-3
