"""Station-plane ground contact (AckermannVanDenBogert2010Force,
EspositoMiller2018Force, MeyerFregly2016Force): the model layer, the lowering
to mh_external_force records of kind 1..3, the device DAE and the reader
mh_eval_contact_forces.

The checker (_contact_ref.py) is a numpy.longdouble restatement of the three
calcContactForceOnStation bodies of the reference's StationPlaneContactForce.h
and calls no library code.  The models are testContact.cpp's point mass (a
massless body on slider tx, a 50 kg body on slider ty along ground y, the
station at its origin; a CoordinateActuator on tx and a control goal make it a
problem mh_create takes) and the double pendulum with a station at (0.3, -0.1,
0) of its second link.  The device's margin is the project's 1e-10 (|want| + 1).

Largest |got - want| / (|want| + 1) of the reader against the checker on an
MI355X (test_reader_force_values_at_the_edges prints them): see DESIGN.md,
"Ground contact"."""
import ctypes as C
import itertools
import math
import subprocess

import numpy as np
import pytest

import _contact_ref as ref
import _lanes
from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.model import (AckermannVanDenBogert2010Force, Axis, Body, Coordinate, CoordinateActuator, DataTable,
                           EspositoMiller2018Force, ExternalForce, Function, Joint, MeyerFregly2016Force, Model,
                           Station, model_from_dict, model_to_dict)
from mocohip.problem import MocoControlGoal, MocoProblem
from mocohip.solver import MocoHipSolver, MocoStudy
from mocohip.tape import write_tape
from test_frame_tracking import _info
from test_muscle_outputs import MH_BUILD, _hip

LD = ref.LD
TOL = 1e-10
MASS, G = 50.0, 9.80665
OPTIMAL_FORCE = 10.0
AVDB, EM, MF = AckermannVanDenBogert2010Force, EspositoMiller2018Force, MeyerFregly2016Force

# the reference's test parameters (testContact.cpp createAVDB / createEspositoMiller / createMeyerFregly) and
# each class's defaults
FORCES = {
    "avdb": lambda: AVDB("contact", "/contact_point", stiffness=1e5, dissipation=1.0, friction_coefficient=0.7),
    "em": lambda: EM("contact", "/contact_point", stiffness=1e5, dissipation=1.0, friction_coefficient=0.7),
    "mf": lambda: MF("contact", "/contact_point", stiffness=1e5, dissipation=1.0),
    "avdb_defaults": lambda: AVDB("contact", "/contact_point"),
    "em_defaults": lambda: EM("contact", "/contact_point"),
    "mf_defaults": lambda: MF("contact", "/contact_point"),
    "em_no_offset": lambda: EM("contact", "/contact_point", stiffness=1e5, dissipation=1.0,
                               friction_coefficient=0.7, depth_offset=0.0),
}
KINDS = {"avdb": 1, "em": 2, "mf": 3}


def point_mass_model(force=None) -> Model:
    """create2DPointMassModel (testContact.cpp:34-70); the ty slider's axis
    is ground y itself, so poses carry no rounding."""
    m = Model("point_mass")
    m.add_body(Body("intermed", 0.0, (0, 0, 0), (0, 0, 0, 0, 0, 0)))
    m.add_body(Body("body", MASS, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
    tx = Coordinate("tx", (-math.inf, math.inf), "translational", path="/tx/tx")
    ty = Coordinate("ty", (-math.inf, math.inf), "translational", path="/ty/ty")
    m.add_joint(Joint.slider("tx", "ground", "intermed", tx))
    m.add_joint(Joint("ty", "intermed", "body", [ty],
                      [Axis(abi.MH_AXIS_TRANSLATION, (0, 1, 0), Function.linear("ty"))]))
    m.add_coordinate_actuator(CoordinateActuator("push", "tx", OPTIMAL_FORCE, path="/push"))
    if force is not None:
        m.add_station(Station("contact_point", "body", (0.0, 0.0, 0.0)))
        m.add_contact_force(force)
    return m


def point_mass(force=None, N=3, scheme="trapezoidal", dynamics="explicit", fd="forward", model=None) -> MocoStudy:
    p = MocoProblem(model or point_mass_model(force))
    p.set_time_bounds(0.0, 0.5)
    p.set_state_info("/tx/tx/value", (-1, 1))
    p.set_state_info("/ty/ty/value", (-0.5, 1))
    p.set_state_info("/tx/tx/speed", (-10, 10))
    p.set_state_info("/ty/ty/speed", (-10, 10))
    p.set_control_info("/push", (-50, 50))
    p.add_goal(MocoControlGoal())
    return MocoStudy(p, MocoHipSolver(num_mesh_intervals=N, transcription_scheme=scheme,
                                      multibody_dynamics_mode=dynamics, optim_finite_difference_scheme=fd))


STATION = (0.3, -0.1, 0.0)


def pendulum(forces=(), N=3, scheme="trapezoidal", dynamics="explicit", fd="forward", mutate=None) -> MocoStudy:
    """configs.double_pendulum with contact forces: (force, body, location)
    each on a station of its own."""
    st = configs.double_pendulum(N, scheme, dynamics)
    st.solver.optim_finite_difference_scheme = fd
    m = st.problem.model
    if mutate:
        mutate(m)
    for i, (f, body, loc) in enumerate(forces):
        m.add_station(Station(f.station.lstrip("/"), body, loc))
        m.add_contact_force(f)
    return st


def _pendulum_force(key, name="contact", station="/contact_point"):
    f = FORCES[key]()
    f.name, f.station = name, station
    return f


def _rel(got, want):
    """|got - want| / (|want| + 1) in long double."""
    want = np.asarray(want, dtype=LD)
    return np.abs(np.asarray(got, dtype=LD) - want) / (np.abs(want) + 1)


def _pm_rows(nlp, yvv, tx=0.25, control=0.0, udot=None):
    """Point-mass rows [t, tx, ty, vtx, vty, control (, udot)] from (y, vy, vx)."""
    rows = np.zeros((len(yvv), 1 + nlp.NI))
    rows[:, 0] = np.linspace(0.0, 0.5, len(yvv))
    rows[:, 1] = tx
    for i, (y, vy, vx) in enumerate(yvv):
        rows[i, 2:5] = y, vx, vy
    rows[:, 5] = control
    if udot is not None:
        rows[:, 6:8] = udot
    return rows


YS = [0.5, 1e-3, 1e-12, +0.0, -0.0, -1e-12, -1e-3, -0.05, -0.17]
VYS = [0.0, 0.5, -0.5, 3.0, -3.0]
VXS = [0.0, 1e-9, -1e-9, 0.05, -0.05, 2.5, -2.5, 50.0, -50.0]
MF_YS = [-0.02, -1e-3, 0.0, 1e-2, 0.3, 0.353, 0.36, 1.0]
EDGE_ROWS = list(itertools.product(YS, VYS, VXS))
MF_ROWS = list(itertools.product(MF_YS, [0.0, -0.5, 3.0], [0.0, 0.05, -2.5]))


# ---- CPU: the model layer and the lowering ---------------------------------------

def _two_contact_pendulum():
    return pendulum([(_pendulum_force("em", "heel", "/heel"), "b0", (0.2, 0.05, 0.0)),
                     (_pendulum_force("mf", "toe", "/toe"), "b1", STATION)])


def test_lowering_records_offsets_and_parameters():
    st = _two_contact_pendulum()
    m = st.problem.model
    times = np.linspace(0.0, 1.0, 6)
    m.add_table(DataTable("grf", times, {k: np.sin(times + i) for i, k in enumerate(("fx", "fy", "fz"))}))
    m.add_external_force(ExternalForce("push", "b0", "grf", force_identifier="f"))
    cm = st.problem.create_rep().compiled
    mm = cm.struct
    assert mm.nexternal == 3 and cm.ncontacts == 2
    table, heel, toe = (mm.external[i] for i in range(3))
    assert (table.kind, table.table, table.force_col) == (0, 0, 0)
    T = cm._tables[0]
    ntab = T.nseg * T.ncol * (T.degree + 1)   # the table coefficients come first
    assert ntab > 0 and mm.ncoefs == ntab + 2 * abi.MH_CONTACT_PARAMS
    assert (heel.kind, heel.body, heel.table, heel.point_col, heel.torque_col, heel.force_col) == \
        (2, 0, -1, -1, -1, ntab)
    assert (toe.kind, toe.body, toe.table, toe.point_col, toe.torque_col, toe.force_col) == (3, 1, -1, -1, -1, ntab + 8)
    coefs = np.ctypeslib.as_array(mm.table_coefs, (mm.ncoefs,))
    assert list(coefs[ntab:ntab + 8]) == [0.2, 0.05, 0.0, 1e5, 1.0, 0.7, 0.05, 0.001]
    assert list(coefs[ntab + 8:]) == [0.3, -0.1, 0.0, 1e5, 1.0, 1.0, 0.05, 1.0]
    # the reference's defaults
    assert AVDB("a", "s").parameters() == [5e7, 1.0, 1.0, 0.05, 0.0]
    assert EM("a", "s").parameters() == [2e6, 1.0, 1.0, 0.05, 0.001]
    assert MF("a", "s").parameters() == [1e4, 1e-2, 1.0, 0.05, 1.0]


def _model_bytes(rep):
    mm = rep.struct.model
    ext = C.string_at(mm.external, C.sizeof(abi.mh_external_force) * mm.nexternal) if mm.nexternal else b""
    return (mm.nexternal, mm.ncoefs, ext, C.string_at(mm.table_coefs, 8 * mm.ncoefs) if mm.ncoefs else b"",
            C.string_at(mm.bodies, C.sizeof(abi.mh_body) * mm.nbodies))


def test_a_model_without_contact_lowers_as_before_and_dicts_round_trip():
    plain = configs.gait10dof18musc(2).problem.create_rep()
    mm = plain.struct.model
    assert all(mm.external[e].kind == 0 and mm.external[e].table >= 0 for e in range(mm.nexternal))
    tables = plain.compiled._tables
    assert mm.ncoefs == sum(tables[t].nseg * tables[t].ncol * (tables[t].degree + 1) for t in range(mm.ntables))
    assert "stations" not in model_to_dict(plain.problem.model)
    assert "contact_forces" not in model_to_dict(plain.problem.model)
    st = _two_contact_pendulum()
    again = model_from_dict(model_to_dict(st.problem.model))
    assert again.contact_forces == st.problem.model.contact_forces
    assert again.stations == st.problem.model.stations
    st2 = configs.double_pendulum(3, "trapezoidal")
    st2.problem.model = again
    assert _model_bytes(st2.problem.create_rep()) == _model_bytes(st.problem.create_rep())


def test_model_layer_refusals():
    m = point_mass_model()
    with pytest.raises(ValueError, match="no body 'nobody'"):
        m.add_station(Station("s", "nobody"))
    m.add_station(Station("s", "body"))
    with pytest.raises(ValueError, match="no station '/t'"):
        m.add_contact_force(AVDB("c", "/t"))
    with pytest.raises(ValueError, match="tangent_velocity_scaling_factor = 0.0 is not positive"):
        m.add_contact_force(AVDB("c", "/s", tangent_velocity_scaling_factor=0.0))
    with pytest.raises(ValueError, match="depth_offset = -1.0 is negative"):
        m.add_contact_force(EM("c", "/s", depth_offset=-1.0))
    m.add_contact_force(MF("c", "s"))
    with pytest.raises(ValueError, match="used twice"):
        m.add_contact_force(AVDB("c", "/s"))
    with pytest.raises(TypeError):
        m.add_contact_force(ExternalForce("e", "body", "t"))


def test_host_model_hash_matches_library_and_covers_the_contact():
    lib = abi.load_mocohip()

    def hashes(st):
        rep = st.problem.create_rep()
        h = C.c_uint64()
        assert lib.mh_model_hash(C.byref(rep.struct.model), C.byref(h)) == 0
        assert h.value == abi.model_hash(rep.struct.model)
        return h.value
    seen = {hashes(point_mass())}
    for key in ("avdb", "em", "mf", "em_no_offset", "avdb_defaults"):   # the kind and the parameter block
        h = hashes(point_mass(FORCES[key]()))
        assert h not in seen, key
        seen.add(h)
    moved = point_mass_model(FORCES["avdb"]())
    moved.stations["/contact_point"].location = (0.0, 0.01, 0.0)
    assert hashes(point_mass(model=moved)) not in seen


def test_layout_query_accepts_contact_with_the_twin_s_layout():
    lib = abi.load_mocohip()
    for make in (lambda f: point_mass(f, scheme="hermite-simpson", dynamics="implicit"),
                 lambda f: pendulum([(f, "b1", STATION)] if f else [])):
        rc0, twin, _ = _info(make(None))
        assert rc0 == 0, lib.mh_last_error().decode()
        for key in KINDS:
            rc, info, _ = _info(make(FORCES[key]()))
            assert rc == 0, lib.mh_last_error().decode()
            assert (info.n, info.m, info.nnz_jac_g) == (twin.n, twin.m, twin.nnz_jac_g)


def test_backend_for_a_contact_model_is_the_generic_interpreter():
    lib = abi.load_mocohip()
    name = C.create_string_buffer(128)
    for st, want in ((configs.double_pendulum(3), "generated:"),
                     (pendulum([(_pendulum_force("avdb"), "b1", STATION)], scheme="hermite-simpson"), "generic")):
        rep, opts = st.problem.create_rep(), st.solver.options()
        assert lib.mh_backend_for(C.byref(rep.struct), C.byref(opts), name, 128) == 0
        assert name.value.decode().startswith(want), name.value


def _bad_records():
    """(mutation of the contact record (external[0]) or its block, message)."""
    def rec(**kw):
        def f(p):
            for k, v in kw.items():
                setattr(p.model.external[0], k, v)
        return f

    def coef(off, v):
        def f(p):
            p.model.table_coefs[p.model.external[0].force_col + off] = v
        return f

    def short(p):
        p.model.ncoefs = p.model.external[0].force_col + 7
    return [
        (rec(kind=4), "unknown kind 4"), (rec(kind=-1), "unknown kind -1"),
        (rec(force_col=-1), "outside table_coefs"), (rec(force_col=1), "outside table_coefs"),
        (short, "outside table_coefs"),
        (coef(6, 0.0), "scaling factor 0 is not positive"), (coef(6, -0.05), "scaling factor -0.05 is not positive"),
        (coef(6, math.nan), "scaling factor nan is not positive"),
        (coef(7, -1e-3), "negative depth_offset -0.001"),
        (rec(table=0), "with a table"),
        (rec(body=2), "bad body"), (rec(body=-1), "bad body"),
    ]


def test_create_validation_refuses_malformed_contact_records():
    lib = abi.load_mocohip()
    for mutate, msg in _bad_records():
        rc, _, _ = _info(point_mass(FORCES["em"]()), mutate)
        err = lib.mh_last_error().decode()
        assert rc == abi.MH_ERR_INVALID and msg in err, (msg, rc, err)
    # a kind-0 record that names no table is still refused
    def table_less(p):
        p.model.external[0].kind = 0
    rc, _, _ = _info(point_mass(FORCES["em"]()), table_less)
    assert rc == abi.MH_ERR_INVALID and "bad body/table" in lib.mh_last_error().decode()
    # MeyerFregly2016 does not read the scaling factor or depth_offset
    def mf_unused(p):
        p.model.table_coefs[p.model.external[0].force_col + 6] = 0.0
    rc, _, _ = _info(point_mass(FORCES["mf"]()), mf_unused)
    assert rc == 0, lib.mh_last_error().decode()


def test_contact_with_prescribed_kinematics_is_unsupported():
    lib = abi.load_mocohip()
    st = configs.gait10dof18musc_inverse(2)
    m = st.problem.model
    body = next(iter(m.bodies))
    m.add_station(Station("heel", body, (0.0, -0.05, 0.0)))
    m.add_contact_force(AVDB("contact", "/heel"))
    rc, _, _ = _info(st)
    err = lib.mh_last_error().decode()
    assert rc == abi.MH_ERR_UNSUPPORTED and "contact with prescribed kinematics" in err, (rc, err)


OSIM = """<?xml version="1.0" encoding="UTF-8" ?>
<OpenSimDocument Version="40000">
  <Model name="point_mass">
    <gravity>0 -9.80665 0</gravity>
    <BodySet><objects>
      <Body name="intermed"><mass>0</mass><mass_center>0 0 0</mass_center><inertia>0 0 0 0 0 0</inertia></Body>
      <Body name="body"><mass>50</mass><mass_center>0 0 0</mass_center><inertia>1 1 1 0 0 0</inertia>
        BODY_PARTS
      </Body>
    </objects></BodySet>
    <JointSet><objects>
      <SliderJoint name="tx">
        <socket_parent_frame>/ground</socket_parent_frame>
        <socket_child_frame>/bodyset/intermed</socket_child_frame>
        <coordinates><Coordinate name="tx"><motion_type>translational</motion_type></Coordinate></coordinates>
      </SliderJoint>
      <CustomJoint name="ty">
        <socket_parent_frame>/bodyset/intermed</socket_parent_frame>
        <socket_child_frame>/bodyset/body</socket_child_frame>
        <coordinates><Coordinate name="ty"><motion_type>translational</motion_type></Coordinate></coordinates>
        <SpatialTransform>
          <TransformAxis name="translation2"><coordinates>ty</coordinates><axis>0 1 0</axis>
            <LinearFunction name="function"><coefficients>1 0</coefficients></LinearFunction>
          </TransformAxis>
        </SpatialTransform>
      </CustomJoint>
    </objects></JointSet>
    <ForceSet><objects>
      <CoordinateActuator name="push"><coordinate>tx</coordinate><optimal_force>10</optimal_force></CoordinateActuator>
      FORCES
    </objects></ForceSet>
    <components>
      COMPONENTS
    </components>
  </Model>
</OpenSimDocument>
"""
OSIM_STATION = """<Station name="contact_point"><socket_parent_frame>/bodyset/body</socket_parent_frame>
        <location>0.01 -0.02 0.03</location></Station>"""
OSIM_FORCES = """
      <AckermannVanDenBogert2010Force name="a"><socket_station>/contact_point</socket_station>
        <stiffness>100000</stiffness><friction_coefficient>0.7</friction_coefficient>
      </AckermannVanDenBogert2010Force>
      <EspositoMiller2018Force name="e">
        <socket_station_connectee_name>/contact_point</socket_station_connectee_name>
        <dissipation>0.5</dissipation><depth_offset>0.002</depth_offset>
        <tangent_velocity_scaling_factor>0.1</tangent_velocity_scaling_factor>
      </EspositoMiller2018Force>
      <MeyerFregly2016Force name="m"><socket_station>/contact_point</socket_station><tscale>2</tscale>
      </MeyerFregly2016Force>"""


@pytest.mark.parametrize("where", ["forceset", "components"])
def test_osim_reads_to_the_same_lowered_bytes(tmp_path, where):
    from mocohip.osim import read_osim
    text = OSIM.replace("FORCES", OSIM_FORCES if where == "forceset" else "")
    if where == "forceset":   # the station among the body's components, the forces in the ForceSet
        text = text.replace("BODY_PARTS", "<components>" + OSIM_STATION + "</components>").replace(
            "COMPONENTS", "")
    else:
        text = text.replace("BODY_PARTS", "").replace("COMPONENTS", OSIM_STATION + OSIM_FORCES)
    path = tmp_path / "m.osim"
    path.write_text(text)
    got = read_osim(str(path))
    want = point_mass_model()
    want.add_station(Station("contact_point", "body", (0.01, -0.02, 0.03)))
    want.add_contact_force(AVDB("a", "/contact_point", stiffness=1e5, friction_coefficient=0.7))
    want.add_contact_force(EM("e", "/contact_point", dissipation=0.5, depth_offset=0.002,
                              tangent_velocity_scaling_factor=0.1))
    want.add_contact_force(MF("m", "/contact_point", tscale=2.0))
    assert [type(f) for f in got.contact_forces] == [AVDB, EM, MF]
    assert _model_bytes(point_mass(model=got).problem.create_rep()) == \
        _model_bytes(point_mass(model=want).problem.create_rep())


@pytest.mark.parametrize("where", ["FORCES", "COMPONENTS"])
def test_osim_still_refuses_smooth_sphere_half_space_force(tmp_path, where):
    from mocohip.osim import read_osim
    text = OSIM.replace(where, '<SmoothSphereHalfSpaceForce name="ball"/>')
    text = text.replace("BODY_PARTS", "").replace("FORCES", "").replace("COMPONENTS", "")
    path = tmp_path / "m.osim"
    path.write_text(text)
    with pytest.raises(NotImplementedError, match="SmoothSphereHalfSpaceForce"):
        read_osim(str(path))


BUILDER_CASES = {
    "point_mass_avdb": lambda: point_mass(FORCES["avdb"]()),
    "point_mass_em_implicit": lambda: point_mass(FORCES["em_defaults"](), scheme="hermite-simpson",
                                                 dynamics="implicit"),
    "pendulum_two_contacts": _two_contact_pendulum,
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    model.py; the description carries one station and one contact record per
    force."""
    st = BUILDER_CASES[name]()
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    lines = desc.read_text().splitlines()
    n = len(st.problem.model.contact_forces)
    assert sum(ln.startswith("contact ") for ln in lines) == n
    assert sum(ln.startswith("station ") for ln in lines) == n
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


def test_oracle_refuses_a_contact_model():
    from mocohip.solver import OracleNLP
    st = point_mass(FORCES["avdb"]())
    with pytest.raises(TypeError, match="contact"):
        OracleNLP(st.problem.create_rep(), st.solver.options())


def test_the_checker_has_the_laws_properties():
    """What the header's formulas imply, held on the checker before the device
    is held to it."""
    a, e, m = FORCES["avdb"](), FORCES["em"](), FORCES["mf"]()
    # AVDB: above ground only the void stiffness; the clamp at 1 + b depthRate < 0
    assert ref.force(a, 0.5, 0.0, 0.0) == (0, LD(-0.5))
    assert ref.force(a, -0.05, 3.0, 0.0)[1] == LD(0.05)
    assert ref.force(e, -0.05, 3.0, 0.0)[1] < 0
    # friction opposes sliding and saturates at mu fy
    fx, fy = ref.force(a, -0.05, 0.0, 50.0)
    assert fx == -LD(0.7) * fy and fy > 0
    fx, fy = ref.force(e, -0.05, 0.0, -50.0)
    assert fx == LD(0.7) * fy
    # EM without an offset: dy is exactly 0 above ground
    assert ref.force(FORCES["em_no_offset"](), 0.25, -1.0, 0.0)[1] == LD(-0.25)
    # MF: zero at ymax by construction, zero past the overflow of double cosh
    assert abs(ref.force(m, 1e-2, 0.0, 0.0)[1]) < 1e-12
    assert ref.force(m, 0.36, -1.0, 1.0) == (0, 0) and ref.force(m, 1.0, 0.0, 0.0)[1] == 0
    assert ref.force(m, 0.353, 0.0, 0.0)[1] != 0
    assert not any(ref.in_mf_band(y) for y in YS + MF_YS)


# ---- GPU -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("key", list(FORCES))
def test_reader_force_values_at_the_edges(key):
    f = FORCES[key]()
    nlp = _hip(point_mass(f))
    assert nlp.backend()[0].startswith("generic"), nlp.backend()
    yvv = EDGE_ROWS + (MF_ROWS if key.startswith("mf") else [])
    rows = _pm_rows(nlp, yvv)
    got = nlp.eval_contact_forces(rows)
    nlp.close()
    assert got.shape == (len(yvv), 1, 9)
    want = ref.forces(f, yvv)
    err = _rel(got[:, 0, :2], want)
    print(f"contact reader [{key}]: largest |got - want| / (|want| + 1) = {float(err.max()):.3e}")
    bad = [(yvv[i], got[i, 0, :2], want[i]) for i in np.nonzero((err > TOL).any(axis=1))[0]]
    assert not bad, bad[:5]
    assert np.all(got[:, 0, 2] == 0.0) and not np.signbit(got[:, 0, 2]).any()
    y, vy, vx = (np.array(c) for c in zip(*yvv))
    assert np.array_equal(got[:, 0, 3], np.full(len(yvv), 0.25)) and np.array_equal(got[:, 0, 4], y)
    assert np.array_equal(got[:, 0, 6], vx) and np.array_equal(got[:, 0, 7], vy)
    assert np.all(got[:, 0, 5] == 0.0) and np.all(got[:, 0, 8] == 0.0)
    if key.startswith("mf"):   # the rows past the overflow of cosh: the force is exactly 0
        off = np.array([(yy + ref.MF_H) / ref.MF_C > ref.COSH_OVERFLOW for yy in y])
        assert off.sum() >= 2 * 9 and np.all(got[off, 0, :2] == 0.0)
    if key == "em_no_offset":   # dy is exactly 0 above ground: the void term alone
        above = (y > 0) & (vx == 0)
        assert np.array_equal(got[above, 0, 1], -y[above])


DAE_ROWS = [(0.5, 0.0, 0.0), (1e-3, -0.5, 0.05), (0.0, 0.5, -0.05), (-0.0, 0.0, 2.5), (-1e-12, -3.0, -2.5),
            (-1e-3, 3.0, 50.0), (-1e-3, -0.5, 1e-9), (-0.05, 0.0, 0.0), (-0.05, 3.0, -50.0), (-0.05, -3.0, 2.5),
            (-0.17, 0.5, -1e-9), (-0.17, -3.0, 0.05), (-0.02, 0.0, -2.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("dynamics", ["explicit", "implicit"])
@pytest.mark.parametrize("key", ["avdb", "em", "mf", "avdb_defaults"])
def test_force_inside_the_dae_on_the_point_mass(key, dynamics):
    f = FORCES[key]()
    nlp = _hip(point_mass(f, dynamics=dynamics))
    want_f = ref.forces(f, DAE_ROWS)
    control = np.linspace(-3.0, 3.0, len(DAE_ROWS))
    udot = np.column_stack([(want_f[:, 0] + LD(OPTIMAL_FORCE) * control.astype(LD)) / LD(MASS),
                            want_f[:, 1] / LD(MASS) - LD(G)])
    if dynamics == "explicit":
        out = nlp.eval_dae(_pm_rows(nlp, DAE_ROWS, control=control))
        err = _rel(out[:, :2], udot)
        assert (err <= TOL).all(), (float(err.max()), out[:, :2], udot)
    else:   # the residual at the closed-form udot, in force units: the bound scaled by m
        closed = udot.astype(float)
        out = nlp.eval_dae(_pm_rows(nlp, DAE_ROWS, control=control, udot=closed))
        bound = TOL * MASS * (np.abs(closed) + 1.0)
        # (closed is udot rounded to double: that rounding, m eps |udot|, is far inside the bound)
        assert (np.abs(out[:, :2]) <= bound).all(), (out[:, :2], bound)
    nlp.close()


def _station_height(q0, q1, loc=STATION):
    a = q0 + q1
    return math.sin(q0) + math.sin(a) + math.sin(a) * loc[0] + math.cos(a) * loc[1]


def _pendulum_rows(nlp, n=10, seed=3):
    """n rows with distinct times, the second link's station between 6 cm in
    the ground and 1 cm above it (q1 by bisection), both links moving."""
    r = np.random.default_rng(seed)
    rows = np.zeros((n, 1 + nlp.NI))
    rows[:, 0] = np.sort(r.uniform(0.0, 1.0, n)) + 0.01 * np.arange(n)
    for i in range(n):
        q0, target = r.uniform(-0.6, -0.2), r.uniform(-0.06, 0.01)
        lo, hi = -0.7, 1.2   # the height rises with q1 on this range
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if _station_height(q0, mid) < target else (lo, mid)
        rows[i, 1:3] = q0, lo
        rows[i, 3:5] = r.uniform(-1.5, 1.5, 2)
        rows[i, 5:7] = r.uniform(-5.0, 5.0, 2)
    return rows


def _twin_with_tables(specs, rows, got):
    """The pendulum without contact but with one ExternalForce per contact,
    whose degree-1 table returns at each row's time the force and the station
    position the reader gave (got [rows, contacts, 9])."""
    t = rows[:, 0]
    br = np.append(t, t[-1] + 1.0)

    def add(m):
        for k, (_, body, _) in enumerate(specs):
            cols = [f"{c}{a}" for c in "fp" for a in "xyz"]
            vals = got[:, k, :6]
            cf = np.zeros((len(t), 6, 2))
            cf[:, :, 0] = vals
            cf[:-1, :, 1] = (vals[1:] - vals[:-1]) / (t[1:] - t[:-1])[:, None]
            m.add_table(DataTable(f"twin{k}", t, {c: vals[:, j].copy() for j, c in enumerate(cols)}, degree=1,
                                  ppoly=(br, cf)))
            m.add_external_force(ExternalForce(f"twin{k}", body, f"twin{k}", force_identifier="f",
                                               point_identifier="p"))
    return pendulum(mutate=add)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["avdb", "em", "mf", "two_contacts"])
def test_force_on_a_rotating_body_equals_the_twin_s_table_force(case):
    if case == "two_contacts":
        specs = [(_pendulum_force("em", "heel", "/heel"), "b0", (0.1, 0.25, 0.0)),
                 (_pendulum_force("avdb", "toe", "/toe"), "b1", STATION)]
    else:
        specs = [(_pendulum_force(case), "b1", STATION)]
    nlp = _hip(pendulum(specs))
    rows = _pendulum_rows(nlp)
    got = nlp.eval_contact_forces(rows)
    out = nlp.eval_dae(rows)
    nlp.close()
    assert got.shape == (len(rows), len(specs), 9)
    # the reader's station kinematics and force against the closed form and the checker
    for k, (f, body, loc) in enumerate(specs):
        for i, row in enumerate(rows):
            q0, q1, u0, u1 = row[1:5]
            a = q0 + (q1 if body == "b1" else 0.0)
            w = u0 + (u1 if body == "b1" else 0.0)
            base = np.array([math.cos(q0), math.sin(q0)]) if body == "b1" else np.zeros(2)
            vbase = u0 * np.array([-math.sin(q0), math.cos(q0)]) if body == "b1" else np.zeros(2)
            arm = np.array([math.cos(a) * (1 + loc[0]) - math.sin(a) * loc[1],
                            math.sin(a) * (1 + loc[0]) + math.cos(a) * loc[1]])
            p, v = base + arm, vbase + w * np.array([-arm[1], arm[0]])
            assert np.all(np.abs(got[i, k, 3:5] - p) <= 1e-12 * 4) and got[i, k, 5] == 0.0
            assert np.all(np.abs(got[i, k, 6:8] - v) <= 1e-12 * 16) and got[i, k, 8] == 0.0
            want = ref.force(f, got[i, k, 4], got[i, k, 7], got[i, k, 6])
            assert (_rel(got[i, k, :2], want) <= TOL).all(), (k, i, got[i, k], want)
    assert (got[:, -1, 4] < 0.011).all() and (got[:, -1, 4] > -0.061).all() and (got[:, -1, 1] != 0).all()
    twin = _hip(_twin_with_tables(specs, rows, got))
    want = twin.eval_dae(rows)
    twin.close()
    err = _rel(out, want)
    assert (err <= TOL).all(), float(err.max())
    plain = _hip(pendulum())
    free = plain.eval_dae(rows)
    plain.close()
    assert (np.abs(out - free) > 1e-3).any()   # the force is felt


def _in_ground_iterate(nlp, model_kind, seed=0):
    """An iterate with the station 2 cm in the ground and sliding at every
    grid point."""
    x = nlp.random_iterate(np.random.default_rng(seed).uniform(-1, 1, nlp.n))
    x[0], x[1] = 0.0, 0.5
    G, NS = nlp.G, nlp.NS
    S = x[2:2 + NS * G].reshape(G, NS)
    r = np.random.default_rng(seed + 1)
    for k in range(G):
        if model_kind == "point_mass":
            S[k] = r.uniform(-0.5, 0.5), -0.02 + r.uniform(-1e-3, 1e-3), r.uniform(0.5, 2.5), r.uniform(-0.3, 0.3)
        else:
            q0 = r.uniform(-0.6, -0.2)
            lo, hi = -0.7, 1.2
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if _station_height(q0, mid) < -0.02 else (lo, mid)
            S[k] = q0, lo, r.uniform(0.5, 1.5), r.uniform(-1.0, 1.0)
    return x


LANE_CASES = [(m, s, fd) for m in ("point_mass", "pendulum") for s in ("trapezoidal", "hermite-simpson")
              for fd in ("forward", "central")]


@pytest.mark.gpu
@pytest.mark.parametrize("model_kind,scheme,fd", LANE_CASES)
def test_lanes_g_and_jacobian_are_the_dae_s_bit_for_bit(model_kind, scheme, fd):
    from mocohip.solver import OracleNLP
    key = ("avdb", "em", "mf")[LANE_CASES.index((model_kind, scheme, fd)) % 3]
    if model_kind == "point_mass":
        st, twin = point_mass(FORCES[key](), 3, scheme, fd=fd), point_mass(None, 3, scheme, fd=fd)
    else:
        st = pendulum([(_pendulum_force(key), "b1", STATION)], 3, scheme, fd=fd)
        twin = pendulum([], 3, scheme, fd=fd)
    nlp = _hip(st)
    assert nlp.backend()[0].startswith("generic"), nlp.backend()
    x = _in_ground_iterate(nlp, model_kind)
    t, Y = nlp.jacobian_lanes(x)
    rows = _lanes.lane_rows(nlp, x, t)
    Gp, S, W = rows.shape
    direct = nlp.eval_dae(rows.reshape(Gp * S, W)).reshape(Gp, S, nlp.NO).transpose(0, 2, 1)
    assert np.array_equal(Y, direct)
    forces = nlp.eval_contact_forces(rows[:, -1, :])
    assert (forces[:, 0, 4] < -0.015).all() and (forces[:, 0, 4] > -0.025).all() and (forces[:, 0, 0] != 0).all()
    orc = OracleNLP(twin.problem.create_rep(), twin.solver.options())
    assert (orc.n, orc.m, orc.nnz) == (nlp.n, nlp.m, nlp.nnz)
    g0, J0 = orc.assemble_from_lanes(x, t, Y)
    orc.close()
    g, J = nlp.eval_g(x), nlp.eval_jac_g(x)
    nlp.close()
    assert np.array_equal(g, g0) and np.array_equal(J, J0)


def _rk4(nlp, state, t_end, dt=2e-3):
    """Classical RK4 of the point mass with the device DAE as the right-hand
    side (one eval_dae row per stage), control 0."""
    def rhs(s):
        row = np.zeros((1, 1 + nlp.NI))
        row[0, 1:5] = s
        return np.concatenate([s[2:], nlp.eval_dae(row)[0, :2]])
    s = np.array(state, float)
    for _ in range(int(round(t_end / dt))):
        k1 = rhs(s)
        k2 = rhs(s + 0.5 * dt * k1)
        k3 = rhs(s + 0.5 * dt * k2)
        k4 = rhs(s + dt * k3)
        s = s + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("key,mu", [("avdb", 0.7), ("em", 0.7), ("mf", 1.0)])
def test_the_reference_s_known_answers_by_rk4_on_the_device_dae(key, mu):
    """testContact.cpp:76-112 (the normal force settles to the weight) and
    :162-207 (the friction distance), time stepping only."""
    nlp = _hip(point_mass(FORCES[key]()))
    s = _rk4(nlp, [0.0, 0.5, 0.0, 0.0], 2.0)
    row = np.zeros((1, 1 + nlp.NI))
    row[0, 1:5] = s
    f = nlp.eval_contact_forces(row)[0, 0]
    print(f"contact rk4 [{key}]: fy / weight = {f[1] / (MASS * G):.5f}, fx = {f[0]:.3e}, height = {s[1]!r}")
    assert abs(f[1] - MASS * G) <= 0.01 * MASS * G and abs(f[0]) <= 0.01 and f[2] == 0.0
    vx0 = 2.5
    e = _rk4(nlp, [0.0, s[1], vx0, 0.0], 0.5)
    nlp.close()
    want = vx0 * vx0 / (2.0 * mu * G)
    print(f"contact rk4 [{key}]: final tx = {e[0]:.5f}, wanted {want:.5f}, end speeds {e[2]:.2e} {e[3]:.2e}")
    assert vx0 / (mu * G) < 0.5
    assert abs(e[0] - want) <= 0.005
    assert abs(e[2]) <= 1e-3 and abs(e[3]) <= 1e-3


@pytest.mark.gpu
def test_frame_accelerations_see_the_contact_force():
    from mocohip.problem import FrameReference, MocoAccelerationTrackingGoal
    f = FORCES["avdb"]()
    st = point_mass(f)
    times = np.linspace(0.0, 0.5, 8)
    g = MocoAccelerationTrackingGoal("acc", 1.0, reference=FrameReference(times, ["/bodyset/body"],
                                                                          np.zeros((8, 1, 3))))
    st.problem.model.add_table(g.reference_table(st.problem.model))
    st.problem.add_goal(g)
    nlp = _hip(st)
    yvv = [(-0.17, -0.2, 1.5)]
    got = nlp.eval_frame_accelerations(list(nlp.rep.goal_names).index("acc"), _pm_rows(nlp, yvv))
    nlp.close()
    fx, fy = ref.force(f, *yvv[0])
    want = np.array([fx / LD(MASS), fy / LD(MASS) - LD(G), LD(0)])
    assert fy > 100 and (_rel(got[0, 0], want) <= TOL).all(), (got, want)


@pytest.mark.gpu
def test_analyze_labels_and_shape():
    st = pendulum([(_pendulum_force("em", "heel", "/heel"), "b0", (0.1, 0.25, 0.0)),
                   (_pendulum_force("avdb"), "b1", STATION)])
    nlp = _hip(st)
    x = _in_ground_iterate(nlp, "pendulum")
    table = st.analyze(x, [r"/forceset/contact\|force_on_station"], nlp)
    base = "/forceset/contact|force_on_station"
    assert list(table.columns) == [base + "_x", base + "_y", base + "_z"]
    rows = np.column_stack([table.times, nlp.point_inputs(x)])
    got = nlp.eval_contact_forces(rows)
    assert len(table.times) == nlp.G
    for i, a in enumerate("xyz"):
        assert np.array_equal(table.columns[f"{base}_{a}"], got[:, 1, i])
    assert (got[:, 1, 1] > 0).all()
    both = st.analyze(x, [r".*\|force_on_station"], nlp)
    assert len(both.columns) == 6 and list(both.columns)[0] == "/forceset/heel|force_on_station_x"
    assert len(st.analyze(x, ["/nothing"], nlp).columns) == 0
    with pytest.raises(RuntimeError, match="0 rows"):
        nlp.eval_contact_forces(rows[:0])
    nlp.close()
