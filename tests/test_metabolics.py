"""Bhargava2004Metabolics: the model component, MocoOutputGoal over its outputs
(goal kind 18), mh_eval_metabolics and MocoStudy.analyze.

The checker (_metabolics_ref.py) is a NumPy restatement of calcMetabolicRate
and its conditionals (Bhargava2004Metabolics.cpp:177-215, 337-537).  It is fed
by test_muscle_outputs' restated_outputs / Checker, which are pinned to the
reference's fixtures through the oracle, and calls no library code under test.
test_the_checker_has_the_reference_s_properties holds it to the properties
testMocoMetabolics.cpp:180-604 checks before the device is held to it.  The
device's margin is the project's 1e-10 (|want| + 1)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _metabolics_ref as ref
from mocohip import abi, configs
from mocohip.describe import write_description
from mocohip.model import Bhargava2004Metabolics, CoordinateActuator
from mocohip.problem import MocoControlGoal, MocoOutputGoal
from mocohip.tape import write_tape
from mocohip.trajectory import read_table, write_table
from test_frame_tracking import _info
from test_marker_tracking import quadrature
from test_muscle_outputs import (EPS, MH_BUILD, NAMES, SLIDER, TOL, Checker, _close, _coupled_muscle_study, _grid_rows,
                                 _hip, _muscle_range, _slider_iterate, _x_index, restated_outputs)

OUT = abi.METABOLICS_OUTPUTS


# ---- 1. the checker is the reference's model -------------------------------------

class _SliderState:
    """The slider muscle (rigid tendon) at a fibre length 0.05 m beyond the
    optimal one, as testMocoMetabolics.cpp:182-189 sets its muscle up."""

    def __init__(self):
        st = configs.hanging_muscle(2)
        self.ck = Checker(st)
        self.mu = st.problem.model.muscles[0]
        self.struct = self.ck.rep.compiled._muscles[0]
        width = self.mu.optimal_fiber_length * math.sin(self.mu.pennation_angle_at_optimal)
        fl = self.mu.optimal_fiber_length + 0.05
        self.L = self.mu.tendon_slack_length + math.sqrt(fl * fl - width * width)
        self.vmax = self.mu.optimal_fiber_length * self.mu.max_contraction_velocity
        self.model = st.problem.model

    def q(self, speed, act=1.0, exc=0.8):
        return dict(zip(NAMES, restated_outputs(self.struct, self.L, speed, act, exc, 0.0, 0.0)))

    def rates(self, comp, speed, act=1.0, exc=0.8):
        comp.muscles = []
        mp = comp.add_muscle("actuator", "/forceset/actuator")
        return ref.muscle_rates(comp, mp, ref.muscle_mass(mp, self.mu), self.mu.max_isometric_force,
                                self.q(speed, act, exc)), ref.muscle_mass(mp, self.mu)


def _family(**common):
    """Non-smooth, tanh and huber components with smoothing 1e6, as the
    reference's test builds them."""
    big = dict(velocity_smoothing=1e6, heat_rate_smoothing=1e6, power_smoothing=1e6)
    return (Bhargava2004Metabolics("n", **common),
            Bhargava2004Metabolics("t", use_smoothing=True, smoothing_type="tanh", **big, **common),
            Bhargava2004Metabolics("h", use_smoothing=True, smoothing_type="huber", **big, **common))


def test_the_checker_has_the_reference_s_properties():
    S = _SliderState()
    assert S.q(0.0)["fiber_length"] == pytest.approx(S.mu.optimal_fiber_length + 0.05, rel=4 * EPS)
    # smooth (1e6) = non-smooth within the reference's 1e-4 over -0.1 .. 0.1 Vmax
    for dep in (False, True):
        fam = _family(include_negative_mechanical_work=False, use_force_dependent_shortening_prop_constant=dep)
        for i in range(-10, 11):
            speed = 0.01 * i * S.vmax
            rn, rt, rh = (S.rates(c, speed)[0] for c in fam)
            for key in ("shortening", "work", "total"):
                assert abs(rn[key] - rt[key]) <= 1e-4 and abs(rn[key] - rh[key]) <= 1e-4, (dep, i, key, rn, rt, rh)
    # work rate 0 at zero speed; activation and maintenance 0 at zero excitation
    for c in _family(include_negative_mechanical_work=False):
        assert abs(S.rates(c, 0.0)[0]["work"]) <= 1e-4
        r0 = S.rates(c, -0.1, exc=0.0)[0]
        assert r0["activation"] == 0.0 and r0["maintenance"] == 0.0
    # work = -scaling * F_active * v in both directions when negative work is allowed
    for c in _family(muscle_effort_scaling_factor=0.9):
        for speed in (-0.1, 0.1):
            q = S.q(speed)
            assert S.rates(c, speed)[0]["work"] == -(0.9 * q["active_fiber_force"]) * q["fiber_velocity"]
    assert S.q(-0.1)["fiber_velocity"] < 0.0 < S.q(0.1)["fiber_velocity"]
    # ... and 0 in eccentric contraction when it is not
    n, t, h = _family(include_negative_mechanical_work=False)
    assert S.rates(n, 0.1)[0]["work"] == 0.0
    assert abs(S.rates(t, 0.1)[0]["work"]) <= 1e-4 and abs(S.rates(h, 0.1)[0]["work"]) <= 1e-4
    # the total power clamps to exactly 0 (eccentric, negative work allowed).  The reference's inputs
    # (activation 0.001, excitation 0.02, speed 0.02) leave the power of this rigid-tendon muscle positive
    # (its compliant muscle shortens against the tendon instead), so there the clamp must do nothing,
    # exactly; full activation at the same low excitation makes the power negative, and the sum exactly 0
    for c in _family():
        r, _ = S.rates(c, 0.02, act=0.001, exc=0.02)
        assert r["power"] > 0.0
        assert r["activation"] + r["maintenance"] + r["shortening"] + r["work"] == r["power"], (c.name, r)
        r, _ = S.rates(c, 0.1, act=1.0, exc=0.02)
        assert r["power"] < 0.0
        assert r["activation"] + r["maintenance"] + r["shortening"] + r["work"] == 0.0, (c.name, r)
    # the total heat clamps to the muscle mass (1 W/kg)
    for c in _family(include_negative_mechanical_work=False):
        r, mass = S.rates(c, 0.02, act=0.001, exc=0.02)
        assert r["heat"] < mass
        assert abs(r["total"] - r["work"] - mass) <= 1e-4
    S.ck.orc.close()


# ---- 2. lowering -----------------------------------------------------------------

def _block(rep, g=0):
    G = rep._goals[g]
    tb, n = G.term_begin, G.term_count
    return list(rep._gidx[tb:tb + n]), list(rep._gcol[tb:tb + n]), list(rep._gw[tb:tb + n])


def test_lowering_term_block():
    st = configs.hanging_muscle_metabolics(2)
    rep = st.problem.create_rep()
    mu = st.problem.model.muscles[0]
    assert abi.MH_GOAL_METABOLICS == 18 and abi.MH_MET_COUNT == 6
    assert (rep._goals[0].kind, rep._goals[0].term_count, rep._goals[0].weight) == (18, 12, 1.0)
    idx, col, w = _block(rep)
    mass = mu.max_isometric_force / 0.25e6 * 1059.7 * mu.optimal_fiber_length
    basal = 1.2 * configs.HANGING_MUSCLE_MASS ** 1.0
    assert idx == [8 | 16 | 32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert col == [0, -1] + [0] * 10
    assert w == [1.0, basal, 1.0, 10.0, 10.0, 10.0, mass, 0.5, 40.0, 133.0, 74.0, 111.0]
    # every option, a provided mass, the divisor, the basal rate's exponent
    st = configs.hanging_muscle_metabolics(
        2, output="total_shortening_rate", divide_by_mass=True, weight=0.3, muscle_mass=0.02,
        ratio_slow_twitch_fibers=0.25, use_smoothing=True, smoothing_type="huber",
        use_force_dependent_shortening_prop_constant=True, include_negative_mechanical_work=False,
        forbid_negative_total_power=False, enforce_minimum_heat_rate_per_muscle=False, basal_coefficient=1.5,
        basal_exponent=0.5, muscle_effort_scaling_factor=0.8, velocity_smoothing=3.0, power_smoothing=4.0,
        heat_rate_smoothing=5.0)
    rep = st.problem.create_rep()
    idx, col, w = _block(rep)
    assert rep._goals[0].weight == 0.3 and idx[0] == 1 | 2 | 4 and col[:2] == [3, -1]
    assert w == [configs.HANGING_MUSCLE_MASS, 1.5 * configs.HANGING_MUSCLE_MASS ** 0.5, 0.8, 3.0, 4.0, 5.0,
                 0.02, 0.25, 40.0, 133.0, 74.0, 111.0]
    # huber without use_smoothing is no flag; tanh smoothing is flag 1 alone
    assert configs.hanging_muscle_metabolics(2, smoothing_type="huber").problem.create_rep()._gidx[0] == 8 | 16 | 32
    assert configs.hanging_muscle_metabolics(2, use_smoothing=True).problem.create_rep()._gidx[0] == 1 | 8 | 16 | 32
    # every output id; the channel by the muscle's name and by its path; /componentset/
    for k, name in enumerate(OUT[:-1]):
        r = configs.hanging_muscle_metabolics(2, output=name).problem.create_rep()
        assert (r._gcol[0], r._gcol[1]) == (k, -1)
    for chan in ("actuator", "/forceset/actuator"):
        r = configs.hanging_muscle_metabolics(2, output="muscle_metabolic_rate:" + chan).problem.create_rep()
        assert (r._gcol[0], r._gcol[1]) == (5, 0)
    st = configs.hanging_muscle_metabolics(2)
    st.problem.goals[0].output_path = "/componentset/metabolics|total_metabolic_rate"
    assert _block(st.problem.create_rep()) == _block(configs.hanging_muscle_metabolics(2).problem.create_rep())


def test_lowering_on_gait_channels_and_shared_muscles():
    st = configs.gait10dof18musc_metabolics(2)
    m = st.problem.model
    assert [type(g) for g in st.problem.goals][-2:] == [MocoOutputGoal, MocoControlGoal]   # before the effort goal
    rep = st.problem.create_rep()
    gi = len(st.problem.goals) - 2
    G = rep._goals[gi]
    assert (G.kind, G.term_count, G.weight) == (18, 6 + 6 * 18, 0.1)
    idx, col, w = _block(rep, gi)
    assert idx[0] == 1 | 8 | 16 | 32 and [idx[6 + 6 * k] for k in range(18)] == list(range(18))
    assert w[0] == sum(float(b.mass) for b in m.bodies.values())
    # a second component that shares muscles, listed in reverse model order
    other = Bhargava2004Metabolics("other")
    for i in (11, 6, 2):
        other.add_muscle(m.muscles[i].name, m.muscles[i].path, ratio_slow_twitch_fibers=0.1 * (i % 7))
    m.add_component(other)
    st.problem.goals.insert(0, MocoOutputGoal("one", 1.0, output_path=f"/other|muscle_metabolic_rate:{m.muscles[6].path}"))
    rep = st.problem.create_rep()
    idx, col, w = _block(rep, 0)
    assert (col[0], col[1]) == (5, 1) and [idx[6 + 6 * k] for k in range(3)] == [11, 6, 2]
    assert rep._goals[1 + gi].term_count == 6 + 6 * 18


def test_host_refusals():
    def study(**kw):
        return configs.hanging_muscle_metabolics(2, **kw)

    def lower(path):
        st = study()
        st.problem.goals = [MocoOutputGoal("o", 1.0, output_path=path)]
        return st.problem.create_rep()
    # the unchanged message for a path that is neither a muscle's nor a metabolics component's
    for bad in ("/bodyset/body|position", "/nothing|total_metabolic_rate"):
        with pytest.raises(ValueError, match="is not a DeGrooteFregly2016Muscle of the model; supported: the outputs "
                                             "length, lengthening_speed"):
            lower(bad)
    with pytest.raises(ValueError, match="no supported output 'total_rate'"):
        lower("/metabolics|total_rate")
    with pytest.raises(ValueError, match="no supported output 'muscle_metabolic_rate'"):
        lower("/metabolics|muscle_metabolic_rate")
    with pytest.raises(ValueError, match="has no muscle 'soleus_r'"):
        lower("/metabolics|muscle_metabolic_rate:soleus_r")
    with pytest.raises(NotImplementedError, match="divide_by_displacement"):
        st = study()
        st.problem.goals[0].divide_by_displacement = True
        st.problem.create_rep()
    m = configs.hanging_muscle(2).problem.model
    m.add_coordinate_actuator(CoordinateActuator("motor", "height", 1.0))

    def comp(**kw):
        c = Bhargava2004Metabolics("metabolics", **{k: v for k, v in kw.items() if k in c_fields})
        c.add_muscle("a", kw.get("path", "/forceset/actuator"), **{k: v for k, v in kw.items() if k in m_fields})
        return c
    c_fields = set(Bhargava2004Metabolics.__dataclass_fields__)
    m_fields = {"ratio_slow_twitch_fibers", "muscle_mass"}
    for kw, msg in ((dict(path="/forceset/nothing"), "no muscle '/forceset/nothing'"),
                    (dict(path="/forceset/motor"), "'/forceset/motor' is a CoordinateActuator, not a DeGrooteFregly"),
                    (dict(ratio_slow_twitch_fibers=1.5), "ratio_slow_twitch_fibers = 1.5 is outside"),
                    (dict(ratio_slow_twitch_fibers=-0.1), "ratio_slow_twitch_fibers = -0.1 is outside"),
                    (dict(muscle_mass=0.0), "muscle 'a': muscle mass 0.0 is not positive"),
                    (dict(muscle_mass=-1.0), "muscle 'a': muscle mass -1.0 is not positive"),
                    (dict(velocity_smoothing=0.0), "velocity_smoothing = 0.0 is not positive"),
                    (dict(power_smoothing=-1.0), "power_smoothing = -1.0 is not positive"),
                    (dict(heat_rate_smoothing=0.0), "heat_rate_smoothing = 0.0 is not positive"),
                    (dict(smoothing_type="cubic"), "unknown smoothing_type 'cubic'")):
        with pytest.raises(ValueError, match=msg):
            m.add_component(comp(**kw))
    twice = comp()
    twice.add_muscle("a", "/forceset/actuator")
    with pytest.raises(ValueError, match="muscle name 'a' is used twice"):
        m.add_component(twice)
    # a model may hold several components, and a muscle may be in several; a component's name only once
    m.add_component(comp())
    second = comp()
    second.name = "second"
    m.add_component(second)
    with pytest.raises(ValueError, match="component name 'second' is used twice"):
        m.add_component(second)
    # the lowering checks again: a component changed after it was added
    st = study()
    st.problem.model.components[0].muscles[0].ratio_slow_twitch_fibers = 2.0
    with pytest.raises(ValueError, match="outside"):
        st.problem.create_rep()


# ---- 3. .osim text ---------------------------------------------------------------

OSIM = """<?xml version="1.0" encoding="UTF-8" ?>
<OpenSimDocument Version="40000">
<Model name="hanging_muscle">
  <gravity>9.81 0 0</gravity>
  <BodySet><objects>
    <Body name="body"><mass>0.5</mass><mass_center>0 0 0</mass_center><inertia>0 0 0 0 0 0</inertia></Body>
  </objects></BodySet>
  <JointSet><objects>
    <SliderJoint name="joint">
      <socket_parent_frame>/ground</socket_parent_frame>
      <socket_child_frame>/bodyset/body</socket_child_frame>
      <coordinates><Coordinate name="height"><motion_type>translational</motion_type><range>0 0.3</range>
      </Coordinate></coordinates>
    </SliderJoint>
  </objects></JointSet>
  <ForceSet><objects>
    <DeGrooteFregly2016Muscle name="actuator">
      <max_isometric_force>30</max_isometric_force><optimal_fiber_length>0.1</optimal_fiber_length>
      <tendon_slack_length>0.05</tendon_slack_length><pennation_angle_at_optimal>0.1</pennation_angle_at_optimal>
      <ignore_tendon_compliance>true</ignore_tendon_compliance><fiber_damping>0.01</fiber_damping>
      <GeometryPath><PathPointSet><objects>
        <PathPoint name="origin"><socket_parent_frame>/ground</socket_parent_frame><location>0 0 0</location></PathPoint>
        <PathPoint name="insertion"><socket_parent_frame>/bodyset/body</socket_parent_frame><location>0 0 0</location>
        </PathPoint>
      </objects></PathPointSet></GeometryPath>
    </DeGrooteFregly2016Muscle>
  </objects></ForceSet>
  COMPONENTS
</Model>
</OpenSimDocument>
"""
OSIM_COMPONENT = """<HOLDER_OPEN>
    <Bhargava2004Metabolics name="metabolics">
      <use_smoothing>true</use_smoothing><smoothing_type>huber</smoothing_type>
      <use_force_dependent_shortening_prop_constant>true</use_force_dependent_shortening_prop_constant>
      <include_negative_mechanical_work>false</include_negative_mechanical_work>
      <basal_coefficient>1.5</basal_coefficient><velocity_smoothing>7</velocity_smoothing>
      <muscle_parameters>
        <Bhargava2004Metabolics_MuscleParameters name="first">
          <socket_muscle>/forceset/actuator</socket_muscle>
          <ratio_slow_twitch_fibers>0.3</ratio_slow_twitch_fibers><specific_tension>300000</specific_tension>
          <maintenance_constant_fast_twitch>100</maintenance_constant_fast_twitch>
        </Bhargava2004Metabolics_MuscleParameters>
        <Bhargava2004Metabolics_MuscleParameters name="second">
          <socket_muscle>/forceset/actuator</socket_muscle>
          <use_provided_muscle_mass>true</use_provided_muscle_mass><provided_muscle_mass>0.03</provided_muscle_mass>
        </Bhargava2004Metabolics_MuscleParameters>
        <Bhargava2004Metabolics_MuscleParameters name="third">
          <socket_muscle>/forceset/actuator</socket_muscle>
          <provided_muscle_mass>0.5</provided_muscle_mass>
        </Bhargava2004Metabolics_MuscleParameters>
      </muscle_parameters>
    </Bhargava2004Metabolics>
  <HOLDER_CLOSE>"""


@pytest.mark.parametrize("holder", ["components", "ComponentSet"])
def test_osim_component_round_trips_to_the_same_lowered_bytes(tmp_path, holder):
    from mocohip.osim import read_osim
    from mocohip.problem import MocoProblem
    opened, closed = (("<components>", "</components>") if holder == "components" else
                      ("<ComponentSet><objects>", "</objects></ComponentSet>"))
    comp = OSIM_COMPONENT.replace("<HOLDER_OPEN>", opened).replace("<HOLDER_CLOSE>", closed)
    with_c, without = tmp_path / "with.osim", tmp_path / "without.osim"
    with_c.write_text(OSIM.replace("COMPONENTS", comp))
    without.write_text(OSIM.replace("COMPONENTS", ""))
    a, b = read_osim(str(with_c)), read_osim(str(without))
    assert len(a.components) == 1 and b.components == []
    c = Bhargava2004Metabolics("metabolics", use_smoothing=True, smoothing_type="huber",
                               use_force_dependent_shortening_prop_constant=True,
                               include_negative_mechanical_work=False, basal_coefficient=1.5, velocity_smoothing=7.0)
    c.add_muscle("first", "/forceset/actuator", ratio_slow_twitch_fibers=0.3, specific_tension=300000.0,
                 maintenance_constant_fast_twitch=100.0)
    c.add_muscle("second", "/forceset/actuator", muscle_mass=0.03)
    c.add_muscle("third", "/forceset/actuator")   # (a provided mass that is not in use)
    b.add_component(c)
    assert a.components[0] == c
    blocks = []
    for m in (a, b):
        p = MocoProblem(m)
        p.set_time_bounds(0.0, 0.5)
        p.add_goal(MocoOutputGoal("met", 1.0, output_path="/metabolics|muscle_metabolic_rate:second",
                                  divide_by_mass=True))
        rep = p.create_rep()
        blocks.append((bytes(rep._goals[0]), np.array(rep._gidx, np.int32).tobytes(),
                       np.array(rep._gcol, np.int32).tobytes(), np.array(rep._gw, float).tobytes()))
    assert blocks[0] == blocks[1] and rep._goals[0].term_count == 6 + 6 * 3 and rep._gcol[1] == 1


# ---- 4. the C++ builder ----------------------------------------------------------

BUILDER_CASES = {
    "slider": lambda: configs.hanging_muscle_metabolics(5, hold=0.15),
    "slider_options_and_channel": lambda: configs.hanging_muscle_metabolics(
        2, tendon="implicit", output="muscle_metabolic_rate:actuator", divide_by_mass=True, muscle_mass=0.02,
        ratio_slow_twitch_fibers=0.3, use_smoothing=True, smoothing_type="huber", basal_exponent=0.7,
        use_force_dependent_shortening_prop_constant=True, include_negative_mechanical_work=False),
    "gait": lambda: configs.gait10dof18musc_metabolics(2),
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_cpp_builder_tape_byte_identical(tmp_path, name):
    """mh_build lowers the description to the same mh_problem bytes as
    problem.py; the description carries one goal metabolics record."""
    st = BUILDER_CASES[name]()
    desc, py_tape, cpp_tape = tmp_path / "s.mhdesc", tmp_path / "py.tape", tmp_path / "cpp.tape"
    write_description(st, str(desc))
    assert sum(ln.startswith("goal metabolics ") for ln in desc.read_text().splitlines()) == 1
    write_tape(st.problem.create_rep(), st.solver.options(), str(py_tape))
    r = subprocess.run([MH_BUILD, str(desc), str(cpp_tape)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert py_tape.read_bytes() == cpp_tape.read_bytes()


# ---- 5. / 12. refusals -----------------------------------------------------------

def _bad_problems():
    """(mutation of the mh_problem of hanging_muscle_metabolics(2), message,
    error code); goal 0 is the metabolics goal, its 12 terms the only ones."""
    bounds = (abi.mh_bounds * 1)()
    targets = (abi.mh_parameter_target * 1)()

    def seta(field, off, v):
        def f(p):
            getattr(p, field)[p.goals[0].term_begin + off] = v
        return f

    def setg(**kw):
        def f(p):
            for k, v in kw.items():
                setattr(p.goals[0], k, v)
        return f

    def parameter(p):   # one parameter: the mass of body 0
        bounds[0].lower, bounds[0].upper = 0.2, 2.0
        targets[0].parameter, targets[0].kind, targets[0].index, targets[0].element = 0, abi.MH_PARAM_BODY_MASS, 0, 0
        p.nparameters, p.nparameter_targets = 1, 1
        p.parameter_bounds, p.parameter_targets = bounds, targets

    I, U = abi.MH_ERR_INVALID, abi.MH_ERR_UNSUPPORTED
    return [
        (setg(term_count=6), "6 terms are not six header terms and six per muscle", I),
        (setg(term_count=11), "11 terms are not six header terms and six per muscle", I),
        (setg(term_count=0), "0 terms are not six header terms and six per muscle", I),
        (setg(term_count=18), "metabolics goal: bad terms", I),
        (setg(term_begin=-1), "metabolics goal: bad terms", I),
        (seta("goal_index", 0, 64), "bad option flags 64", I),
        (seta("goal_index", 0, -1), "bad option flags -1", I),
        (seta("goal_index", 0, 2), "bad option flags 2", I),
        (seta("goal_column", 0, 6), "output 6 out of range", I),
        (seta("goal_column", 0, -1), "output -1 out of range", I),
        (seta("goal_column", 1, 0), "channel 0 does not fit output 0", I),
        (seta("goal_column", 0, 5), "channel -1 does not fit output 5", I),
        (seta("goal_index", 6, 1), "muscle 1 out of range", I),
        (seta("goal_index", 6, -1), "muscle -1 out of range", I),
        (seta("goal_index", 1, 3), "term 1: an unused index or column is not 0", I),
        (seta("goal_index", 7, 1), "term 7: an unused index or column is not 0", I),
        (seta("goal_column", 7, 1), "term 7: an unused index or column is not 0", I),
        (seta("goal_weight", 0, 0.0), "divisor 0 is not positive and finite", I),
        (seta("goal_weight", 0, math.inf), "divisor inf is not positive and finite", I),
        (seta("goal_weight", 1, math.nan), "basal rate nan is not finite", I),
        (seta("goal_weight", 2, math.inf), "scaling factor inf is not finite", I),
        (seta("goal_weight", 3, 0.0), "smoothing 0 is not positive and finite", I),
        (seta("goal_weight", 4, -1.0), "smoothing -1 is not positive and finite", I),
        (seta("goal_weight", 5, math.nan), "smoothing nan is not positive and finite", I),
        (seta("goal_weight", 6, 0.0), "muscle mass 0 is not positive and finite", I),
        (seta("goal_weight", 7, 1.5), "slow-twitch ratio 1.5 is outside", I),
        (seta("goal_weight", 7, math.nan), "slow-twitch ratio nan is outside", I),
        (seta("goal_weight", 9, math.inf), "heat constant inf is not finite", I),
        (parameter, "metabolics goal with MocoParameters", U),
    ]


def test_layout_query_accepts_the_goal_and_refuses_what_create_refuses():
    lib = abi.load_mocohip()
    for st in (configs.hanging_muscle_metabolics(2), configs.gait10dof18musc_metabolics(2),
               configs.hanging_muscle_metabolics(2, tendon="implicit", output="muscle_metabolic_rate:actuator")):
        rc, info, _ = _info(st)
        assert rc == 0, lib.mh_last_error().decode()
    for mutate, msg, code in _bad_problems():
        rc, _, _ = _info(configs.hanging_muscle_metabolics(2), mutate)
        err = lib.mh_last_error().decode()
        assert rc == code and msg in err and err.startswith("goal 0: "), (msg, rc, err)


@pytest.mark.gpu
def test_refusals_and_the_reader_s_own():
    from mocohip.solver import HipNLP
    I, U = abi.MH_ERR_INVALID, abi.MH_ERR_UNSUPPORTED
    lib = abi.load_mocohip()
    for mutate, msg, code in _bad_problems():
        st = configs.hanging_muscle_metabolics(2)
        rep = st.problem.create_rep()
        mutate(rep.struct)
        _info(st, mutate)
        want = lib.mh_last_error().decode()   # mh_get_nlp_info_for's message
        with pytest.raises(RuntimeError) as e:
            HipNLP(rep, st.solver.options())
        assert f"error {code}: " in str(e.value) and msg in str(e.value) and want in str(e.value), (str(e.value), want)
    st = configs.hanging_muscle(2)   # no metabolics goal: the reader is not tied to one
    comp = configs.hanging_muscle_metabolics(2).problem.model.components[0]
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    rows = np.zeros((1, 1 + nlp.NI))
    rows[0, 1:] = (0.15, -0.1, 0.5, 0.4)
    assert nlp.eval_metabolics(comp, rows).shape == (1, 6)
    idx, col, w = comp.term_block(st.problem.model)
    with pytest.raises(RuntimeError, match=f"error {I}: .*0 rows"):
        nlp.eval_metabolics_block(idx, col, w, rows[:0])
    for field, off, v, msg in ((idx, 6, 1, "muscle 1 out of range"), (idx, 0, 64, "bad option flags 64"),
                               (col, 0, 6, "output 6 out of range"), (w, 6, 0.0, "muscle mass 0 is not positive"),
                               (w, 3, -1.0, "smoothing -1 is not positive")):
        bad = [list(idx), list(col), list(w)]
        bad[[idx, col, w].index(field)][off] = v
        with pytest.raises(RuntimeError, match=f"error {I}: mh_eval_metabolics: .*{msg}"):
            nlp.eval_metabolics_block(*bad, rows)
    for n in (0, 6, 11):
        with pytest.raises(RuntimeError, match=f"error {I}: .*{n} terms are not six header terms"):
            nlp.eval_metabolics_block(idx[:n], col[:n], w[:n], rows)
    nlp.close()
    st = configs.gait10dof18musc_parameters(2)
    nlp = HipNLP(st.problem.create_rep(), st.solver.options())
    c = Bhargava2004Metabolics("m")
    c.add_muscle("a", st.problem.model.muscles[0].path)
    with pytest.raises(RuntimeError, match=f"error {U}: .*mh_eval_metabolics with MocoParameters"):
        nlp.eval_metabolics(c, np.zeros((1, 1 + nlp.NI)))
    nlp.close()


# ---- 6. reader values against the checker ----------------------------------------

MODES = {"none": dict(), "tanh": dict(use_smoothing=True, smoothing_type="tanh"),
         "huber": dict(use_smoothing=True, smoothing_type="huber")}


def _components(muscles, model):
    """mode x force-dependent constant x negative work: 12 components over
    ``muscles`` (indices into the model's), smoothing 10."""
    out = []
    for mode, kw in MODES.items():
        for dep in (False, True):
            for neg in (False, True):
                c = Bhargava2004Metabolics(f"{mode}_{int(dep)}{int(neg)}", include_negative_mechanical_work=neg,
                                           use_force_dependent_shortening_prop_constant=dep, **kw)
                for k, i in enumerate(muscles):
                    c.add_muscle(model.muscles[i].name, model.muscles[i].path,
                                 ratio_slow_twitch_fibers=0.5 if len(muscles) == 1 else 0.2 + 0.07 * (k % 9))
                out.append(c)
    return out


def _well_separated(comp, ck, rows):
    """The conditioning rule of the non-smooth and huber modes, on the
    restatement alone: every muscle at every row keeps |fibre velocity| >=
    1e-3 m/s, |power before its clamp| >= 1e-6 W, |heat - mass| >= 1e-6 W."""
    for row in rows:
        for mp, r in zip(comp.muscles, ref.component_rates(comp, ck, row)):
            im = ref.model_muscle(ck.model, mp)
            v = dict(zip(NAMES, ck.outputs(im, row)))["fiber_velocity"]
            mass = ref.muscle_mass(mp, ck.model.muscles[im])
            assert abs(v) >= 1e-3 and abs(r["power"]) >= 1e-6 and abs(r["heat"] - mass) >= 1e-6, \
                (comp.name, mp.name, v, r["power"], r["heat"] - mass)


def _check_reader(nlp, ck, comps, rows, tanh_rows=None, worst=None):
    for comp in comps:
        use = rows
        if comp.use_smoothing and comp.smoothing_type == "tanh":
            use = rows if tanh_rows is None else np.vstack([rows, tanh_rows])
        else:
            _well_separated(comp, ck, rows)
        got = nlp.eval_metabolics(comp, use)
        want = np.array([ref.component_outputs(comp, ck, r) for r in use])
        assert got.shape == want.shape == (len(use), 5 + len(comp.muscles))
        err = float((np.abs(got - want) / (np.abs(want) + 1.0)).max())
        if worst is not None:
            worst[ref.mode_of(comp)] = max(worst.get(ref.mode_of(comp), 0.0), err)
        bad = [(comp.name, r, k, got[r, k], want[r, k]) for r, k in zip(*np.nonzero(~_close(got, want)))]
        assert not bad, bad


def _slider_met_rows(nlp, ck):
    """Four well-separated rows (shortening, lengthening, and two of low
    effort on either side of the clamps) and, for the tanh mode, two rows at
    rest: speed (and tendon-force derivative) exactly 0."""
    rows = np.zeros((6, 1 + nlp.NI))
    rows[:, 0] = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    rows[:, 1] = (0.150, 0.158, 0.162, 0.155, 0.166, 0.152)
    rows[:, 2] = (-0.20, 0.15, 0.05, -0.03, 0.0, 0.0)
    sa, ic, sf, idf = ck.indices(0)
    if sa >= 0:
        rows[:, 1 + sa] = (0.30, 0.55, 0.02, 0.05, 0.80, 0.02)
    rows[:, 1 + ic] = (0.25, 0.60, 0.03, 0.02, 0.70, 0.01)
    if sf >= 0:
        rows[:, 1 + sf] = (0.20, 0.70, 0.10, 0.05, 0.50, 0.03)
    if sf >= 0 and idf < 0:
        # explicit tendon dynamics: the fibre velocity follows from the force balance; tendon forces
        # that keep it moderate at the low activations (0.05, -0.03, 0.004, -0.002 m/s in rows 2 .. 5)
        rows[2:, 1 + sf] = (0.06042, 0.07047, 0.78799, 0.04053)
    if idf >= 0:
        rows[:, 1 + idf] = (0.5, -0.4, 0.2, -0.1, 0.0, 0.0)
    return rows[:4], rows[4:]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(SLIDER))
def test_all_outputs_on_the_slider(variant):
    """All six outputs (the five totals and the muscle's rate: the reader's
    row) in mode x force-dependent constant x negative work."""
    st = configs.hanging_muscle(2, **SLIDER[variant])
    nlp, ck = _hip(st), Checker(st)
    rows, rest = _slider_met_rows(nlp, ck)
    comps = _components([0], st.problem.model)
    worst = {}
    _check_reader(nlp, ck, comps, rows, rest, worst)
    print("slider", variant, "max error / (|want| + 1):", worst)
    # the tanh rows cross each transition: both signs of the fibre velocity, of
    # the power before its clamp and of heat - mass
    tanh = next(c for c in comps if c.name == "tanh_01")
    sig = {"v": set(), "power": set(), "heat": set()}
    for row in np.vstack([rows, rest]):
        r = ref.component_rates(tanh, ck, row)[0]
        q = dict(zip(NAMES, ck.outputs(0, row)))
        mass = ref.muscle_mass(tanh.muscles[0], st.problem.model.muscles[0])
        sig["v"].add(np.sign(q["fiber_velocity"]))
        sig["power"].add(np.sign(r["power"]))
        sig["heat"].add(np.sign(r["heat"] - mass))
    assert sig["v"] >= {-1.0, 1.0} and sig["power"] == {-1.0, 1.0} and sig["heat"] == {-1.0, 1.0}, sig
    if variant != "compliant_explicit":   # (there the fibre velocity follows from the force balance)
        assert 0.0 in sig["v"]
    nlp.close(); ck.orc.close()


def _gait_rows(nlp, seed):
    x = _muscle_range(nlp, np.random.default_rng(seed))
    x[0], x[1] = 0.3, 1.2
    return x, _grid_rows(nlp, x)


@pytest.mark.gpu
def test_gait_components_against_the_checker():
    """gait10dof18musc, N = 2: a component over three non-adjacent muscles in
    reverse model order, then two components that share a muscle."""
    st = configs.gait10dof18musc(2)
    m = st.problem.model
    assert len(m.muscles) == 18
    nlp, ck = _hip(st), Checker(st)
    _, rows = _gait_rows(nlp, 21)
    rows = rows[:3]
    worst = {}
    _check_reader(nlp, ck, _components([11, 6, 2], m), rows, worst=worst)
    for mode, kw in MODES.items():
        a, b = Bhargava2004Metabolics("a", **kw), Bhargava2004Metabolics("b", basal_coefficient=0.7, **kw)
        for i in (4, 9):
            a.add_muscle(m.muscles[i].name, m.muscles[i].path)
        for i in (9, 15, 0):
            b.add_muscle(m.muscles[i].name, m.muscles[i].path, ratio_slow_twitch_fibers=0.8)
        _check_reader(nlp, ck, [a, b], rows, worst=worst)
    print("gait max error / (|want| + 1):", worst)
    nlp.close(); ck.orc.close()


@pytest.mark.gpu
def test_rajagopal_prescribed_wrapped_against_the_checker():
    st = configs.rajagopal18_inverse(1, keep_path_wraps=True)
    m = st.problem.model
    nlp, ck = _hip(st), Checker(st)
    # three rows built here, so that the conditioning rule can be tried on the CPU: times inside the
    # kinematics table, the muscle states, controls and derivative variables in the muscles' range
    r = np.random.default_rng(40)
    nt = len(ck.implicit_tendon)
    lo = 1 + ck.NS + ck.NC
    assert nlp.NI >= ck.NS + ck.NC + nt
    rows = np.zeros((3, 1 + nlp.NI))
    rows[:, 0] = (0.5, 0.7, 0.7321)
    rows[:, 1:1 + ck.NS] = r.uniform(0.05, 0.5, (3, ck.NS))
    rows[:, 1 + ck.NS:lo] = r.uniform(0.05, 0.4, (3, ck.NC))
    rows[:, lo:lo + nt] = r.uniform(-0.5, 0.5, (3, nt))                          # the tendon-force derivatives
    rows[:, lo + nt:] = r.uniform(-0.5, 0.5, (3, 1 + nlp.NI - lo - nt))          # (inputs no muscle reads)
    assert any(len(mu.path_wraps) for mu in m.muscles)
    comps = [c for c in _components(list(range(len(m.muscles))), m) if c.name.endswith("01")]
    worst = {}
    _check_reader(nlp, ck, comps, rows, worst=worst)
    print("rajagopal18 max error / (|want| + 1):", worst)
    nlp.close(); ck.orc.close()


# ---- 7. f and grad f -------------------------------------------------------------

def _goal_value(comp, ck, row, output, channel=-1):
    o = ref.component_outputs(comp, ck, row)
    return o[5 + channel] if output == 5 else o[output]


F_CASES = [("rigid", "hermite-simpson", "central", "tanh", True, "total_metabolic_rate"),
           ("rigid", "trapezoidal", "forward", "huber", False, "total_shortening_rate"),
           ("implicit", "hermite-simpson", "backward", "tanh", True, "total_mechanical_work_rate"),
           ("explicit", "trapezoidal", "central", "tanh", False, "muscle_metabolic_rate:actuator"),
           ("rigid", "hermite-simpson", "forward", "none", False, "total_metabolic_rate"),
           ("rigid", "trapezoidal", "backward", "tanh", False, "total_activation_rate")]


def _check_f_and_grad(st, comp, output, channel, by_mass, seed_x, live_of):
    """f = weight dur sum quad_k L_k with L = value / divisor; grad f at the
    point inputs the goal reads = k_grad's quotient of the checker's L.  The
    device's lane values are each within E_k = 1e-10 (|value| + 1) / divisor of
    the checker's, so a quotient of two of them differs by at most 2 E_k / h
    (forward, backward) or 2 E_k / (2 h) (central), times weight dur quad_k.
    The value does not read the time here, so grad f along t0 / tf is -/+ f /
    dur.  Every other entry is 0: the goal is the only one."""
    nlp, ck = _hip(st), Checker(st)
    weight = st.problem.goals[0].weight
    fd = st.solver.optim_finite_difference_scheme
    x = seed_x(nlp)
    rows = _grid_rows(nlp, x)
    _, quad = quadrature(nlp)
    dur, h = x[1] - x[0], float(nlp.opts.fd_step)
    assert h == 1e-8
    den = sum(float(b.mass) for b in st.problem.model.bodies.values()) if by_mass else 1.0
    if not comp.use_smoothing:
        _well_separated(comp, ck, rows)
    val = lambda r: _goal_value(comp, ck, r, output, channel)   # noqa: E731
    vals = np.array([val(r) for r in rows])
    f = weight * dur * float(quad @ vals) / den
    E = TOL * (np.abs(vals) + 1.0) / den
    got_f = nlp.eval_f(x)
    assert abs(got_f - f) <= weight * dur * float(quad @ E) + 16 * EPS * abs(f), (got_f, f)
    grad = nlp.eval_grad_f(x)
    assert np.array_equal(grad, nlp.eval_grad_f(x)) and got_f == nlp.eval_f(x)   # the same bits on every run
    touched = set()
    worst = 0.0
    for k in range(nlp.G):
        for j in live_of(ck):
            rp, rm = rows[k].copy(), rows[k].copy()
            rp[1 + j] = rows[k][1 + j] + h
            rm[1 + j] = rows[k][1 + j] - h
            dL = {"central": lambda: (val(rp) - val(rm)) / (2.0 * h), "forward": lambda: (val(rp) - vals[k]) / h,
                  "backward": lambda: (vals[k] - val(rm)) / h}[fd]()
            want = weight * dur * quad[k] * dL / den
            bound = weight * dur * quad[k] * 2.0 * E[k] / (2.0 * h if fd == "central" else h)
            i = _x_index(nlp, k, j)
            touched.add(i)
            worst = max(worst, abs(grad[i] - want) / (bound + 16 * EPS * abs(want)))
            assert abs(grad[i] - want) <= bound + 16 * EPS * abs(want), (k, j, grad[i], want, bound)
    print("grad f: worst |error| / bound =", worst)
    assert abs(grad[0] + got_f / dur) <= 1e-12 * abs(got_f / dur) + weight * float(quad @ E)
    assert abs(grad[1] - got_f / dur) <= 1e-12 * abs(got_f / dur) + weight * float(quad @ E)
    rest = np.array([i for i in range(2, nlp.n) if i not in touched], dtype=int)
    assert (grad[rest] == 0.0).all()
    nlp.close(); ck.orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tendon,scheme,fd,mode,by_mass,output", F_CASES)
def test_objective_and_gradient_against_the_checker(tendon, scheme, fd, mode, by_mass, output):
    """The slider: one goal of a single muscle; G x stride (7 x 7, 4 x 11, ...)
    is no multiple of 64, so the last block has a tail."""
    st = configs.hanging_muscle_metabolics(3, output=output, divide_by_mass=by_mass, weight=1.3, tendon=tendon,
                                           scheme=scheme, fd_scheme=fd,
                                           dynamics="implicit" if tendon == "implicit" else "explicit", **MODES[mode])
    comp = st.problem.model.components[0]
    which = OUT.index(output.partition(":")[0])

    def live(ck):
        sa, ic, sf, idf = ck.indices(0)
        return [0, 1] + [j for j in (sa, sf, idf) if j >= 0] + [ic]   # (the excitation control always)
    _check_f_and_grad(st, comp, which, 0 if which == 5 else -1, by_mass, _slider_iterate, live)


@pytest.mark.gpu
def test_objective_and_gradient_of_three_gait_muscles():
    """Three muscles in one goal, more than one block of lanes, forward
    differences: a muscle a direction cannot change enters the sum with its
    base-lane value."""
    st = configs.gait10dof18musc(1, fd_scheme="forward")
    m = st.problem.model
    comp = Bhargava2004Metabolics("metabolics", use_smoothing=True)
    for i in (11, 6, 2):
        comp.add_muscle(m.muscles[i].name, m.muscles[i].path, ratio_slow_twitch_fibers=0.3 + 0.1 * (i % 3))
    m.add_component(comp)
    st.problem.goals = [MocoOutputGoal("met", 0.1, output_path="/metabolics|total_metabolic_rate",
                                       divide_by_mass=True)]

    def seed(nlp):
        x = _muscle_range(nlp, np.random.default_rng(23))
        x[0], x[1] = 0.3, 1.2
        return x

    def live(ck):
        out = list(range(2 * ck.nq))
        for i in (11, 6, 2):
            sa, ic, sf, idf = ck.indices(i)
            out += [j for j in (sa, sf, idf) if j >= 0] + [ic]
        return out
    _check_f_and_grad(st, comp, 0, -1, True, seed, live)


# ---- 8. bit-exact checks ---------------------------------------------------------

def _gait_goal_study(N=1, scheme="trapezoidal", muscles=range(18), weight=0.1, by_mass=False, extra=(), **kw):
    st = configs.gait10dof18musc(N, fd_scheme="forward", **kw)
    st.solver.transcription_scheme = scheme
    m = st.problem.model
    comp = Bhargava2004Metabolics("metabolics", use_smoothing=True)
    for i in muscles:
        comp.add_muscle(m.muscles[i].name, m.muscles[i].path)
    m.add_component(comp)
    st.problem.goals = [MocoOutputGoal("met", weight, output_path="/metabolics|total_metabolic_rate",
                                       divide_by_mass=by_mass)] + list(extra)
    return st


@pytest.mark.gpu
def test_back_ends_and_repeats_bit_identical():
    st = _gait_goal_study(2, "hermite-simpson", by_mass=True)
    runs = []
    for generic in (False, True):
        nlp = _hip(st, generic)
        assert nlp.backend()[0].startswith("generic" if generic else "generated:"), nlp.backend()
        x, _ = _gait_rows(nlp, 31)
        runs.append((nlp.eval_f(x), nlp.eval_grad_f(x), nlp.eval_f(x), nlp.eval_grad_f(x)))
        nlp.close()
    for f, g, f2, g2 in runs:
        assert f == f2 and g.tobytes() == g2.tobytes()
    assert runs[0][0] == runs[1][0] and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert runs[0][0] != 0.0 and np.count_nonzero(runs[0][1]) > 0


@pytest.mark.gpu
def test_pruned_lanes_have_the_bits_of_every_muscle_in_every_lane():
    """One gait grid point (trapezoidal, N = 1: quad = 1/2 exactly), forward
    differences, divisor 1.  The reader evaluates all 18 muscles at the row
    perturbed along each point input, in the kernel's arithmetic (input + h);
    the goal's lanes evaluate only the muscles a direction can change and take
    the others from the base lane.  grad f = weight dur quad (L1 - L0) / h has
    the same bits either way."""
    st = _gait_goal_study(1, "trapezoidal")
    nlp = _hip(st)
    comp = st.problem.model.components[0]
    x, rows = _gait_rows(nlp, 33)
    _, quad = quadrature(nlp)
    assert nlp.G == 2 and quad[0] == 0.5 and quad[1] == 0.5
    grad = nlp.eval_grad_f(x)
    dur, h, w = x[1] - x[0], float(nlp.opts.fd_step), 0.1
    k = 1
    ND = nlp.NS + nlp.NC
    pert = np.repeat(rows[k][None, :], ND + 1, axis=0)
    for j in range(ND):
        pert[j, 1 + j] = rows[k][1 + j] + h
    L = nlp.eval_metabolics(comp, pert)[:, 0]
    moved = 0
    for j in range(ND):
        want = w * dur * quad[k] * ((L[j] - L[ND]) / h)
        got = grad[_x_index(nlp, k, j)]
        assert got.tobytes() == np.float64(want).tobytes(), (j, got, want)
        moved += want != 0.0
    assert moved >= 2 * nlp.NQ + 18
    nlp.close()


# ---- 9. goals combine as independent terms ---------------------------------------

@pytest.mark.gpu
def test_goals_add_up():
    """The metabolics goal, a kind-17 goal and a MocoControlGoal: f and grad f
    equal the sum of the single-goal runs to the rounding of the sums."""
    pm = configs.gait10dof18musc_model().muscles[3].path
    gb = MocoOutputGoal("b", 2.0, output_path=pm + "|fiber_active_power")
    gc = MocoControlGoal("effort", 0.3)
    runs, x = {}, None
    for name, which in (("all", "abc"), ("a", "a"), ("b", "b"), ("c", "c")):
        st = _gait_goal_study(2, "hermite-simpson", muscles=(11, 6, 2), by_mass=True,
                              extra=[g for g, n in ((gc, "c"), (gb, "b")) if n in which])
        if "a" not in which:
            st.problem.goals = st.problem.goals[1:]
        nlp = _hip(st)
        if x is None:
            x, _ = _gait_rows(nlp, 9)
        runs[name] = (nlp.eval_f(x), nlp.eval_grad_f(x))
        nlp.close()
    fs = runs["a"][0] + runs["b"][0] + runs["c"][0]
    mag = abs(runs["a"][0]) + abs(runs["b"][0]) + abs(runs["c"][0])
    assert runs["a"][0] != 0.0 and abs(runs["all"][0] - fs) <= 8 * EPS * mag
    gs = runs["a"][1] + runs["b"][1] + runs["c"][1]
    gm = np.abs(runs["a"][1]) + np.abs(runs["b"][1]) + np.abs(runs["c"][1])
    assert (np.abs(runs["all"][1] - gs) <= 8 * EPS * gm).all()


def _with_metabolics(st, muscle_path):
    comp = Bhargava2004Metabolics("metabolics", use_smoothing=True)
    comp.add_muscle("m", muscle_path)
    st.problem.model.add_component(comp)
    st.problem.goals.insert(0, MocoOutputGoal("met", 1.5, output_path="/metabolics|total_metabolic_rate"))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("dynamics", ["explicit", "implicit"])
def test_untouched_multiplier_slack_and_acceleration_entries(dynamics):
    """test_muscle_outputs' coupled pendulum with a muscle: the multiplier,
    slack and (implicit dynamics) acceleration entries of grad f carry the bits
    of the problem without the goal; the coordinates' entries move."""
    a = _hip(_with_metabolics(_coupled_muscle_study(dynamics, False), "/forceset/flexor"))
    b = _hip(_coupled_muscle_study(dynamics, False))
    assert (a.n, a.NM, a.NSL, a.NDV) == (b.n, b.NM, b.NSL, b.NDV)
    G, N = a.G, a.opts.num_mesh_intervals
    assert a.NM * G > 0 and a.NSL * N > 0 and (a.NDV * G > 0) == (dynamics == "implicit")
    r = np.random.default_rng(12)
    x = a.random_iterate(r.uniform(-1, 1, a.n))
    x[0], x[1] = 0.1, 0.9
    x[2:2 + a.NS * G].reshape(G, a.NS)[:, 4:] = r.uniform(0.2, 0.8, (G, a.NS - 4))   # activations
    ga, gb = a.eval_grad_f(x), b.eval_grad_f(x)
    XM = 2 + (a.NS + a.NC) * G
    XL = XM + a.NM * G
    DB = XL + a.NSL * N
    assert DB + a.NDV * G == a.n
    assert (gb[XM:XL] != 0.0).all()   # (the multiplier goal's)
    assert ga[XM:XL].tobytes() == gb[XM:XL].tobytes()          # multipliers
    assert ga[XL:DB].tobytes() == gb[XL:DB].tobytes()          # slacks
    assert ga[DB:].tobytes() == gb[DB:].tobytes()              # accelerations
    dq = (ga[2:2 + a.NS * G] - gb[2:2 + a.NS * G]).reshape(G, a.NS)
    # both coordinates move the muscle's length (past the first grid point, where the iterate sits on
    # the initial bounds, at rest: the quotients along the two coordinates are exact zeros there)
    assert (dq[1:, :2] != 0.0).all()
    a.close(); b.close()


@pytest.mark.gpu
def test_untouched_acceleration_and_other_muscles_entries_on_gait():
    """Implicit dynamics on the gait model: the acceleration variables' entries
    and the states and controls of the muscles outside the component keep the
    bits of the problem without the goal."""
    a = _hip(_with_metabolics(configs.gait10dof18musc(2, dynamics="implicit"), "/forceset/soleus_r"))
    b = _hip(configs.gait10dof18musc(2, dynamics="implicit"))
    x, _ = _gait_rows(a, 10)
    ga, gb = a.eval_grad_f(x), b.eval_grad_f(x)
    lo = 2 + (a.NS + a.NC) * a.G
    assert a.n - lo >= a.NQ * a.G > 0
    assert ga[lo:].tobytes() == gb[lo:].tobytes()
    sn, cn = a.rep.state_names, a.rep.control_names
    keep_s = [j for j, n in enumerate(sn) if n.startswith("/forceset/") and not n.startswith("/forceset/soleus_r/")]
    keep_c = [j for j, n in enumerate(cn) if n != "/forceset/soleus_r"]
    assert keep_s and keep_c
    for k in range(a.G):
        for j in keep_s:
            assert ga[2 + k * a.NS + j].tobytes() == gb[2 + k * a.NS + j].tobytes(), (k, sn[j])
        for j in keep_c:
            i = 2 + a.NS * a.G + k * a.NC + j
            assert ga[i].tobytes() == gb[i].tobytes(), (k, cn[j])
    ic = 2 + a.NS * a.G + cn.index("/forceset/soleus_r")
    # the excitation's entries move (not where the power clamp holds the rate at 0 whatever the excitation)
    assert any(ga[ic + k * a.NC] != gb[ic + k * a.NC] for k in range(a.G))
    a.close(); b.close()


# ---- 10. shards, 11. batches -----------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 3])
def test_shards_sum_to_the_whole(W):
    N = 3

    def study():
        st = configs.hanging_muscle_metabolics(N, tendon="explicit", fd_scheme="central", weight=1.1,
                                               divide_by_mass=True, use_smoothing=True)
        st.problem.goals.append(MocoControlGoal("effort", 0.2))
        return st
    whole = _hip(study())
    x = _slider_iterate(whole)
    f, grad = whole.eval_f(x), whole.eval_grad_f(x)
    whole.close()
    cuts = [0, 1, 3] if W == 2 else [0, 1, 2, 3]
    fp, gp = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sh = _hip(study(), interval=(lo, hi))
        fp.append(sh.eval_f_partial(x)); gp.append(sh.eval_grad_f_partial(x))
        sh.close()
    assert all(v != 0.0 for v in fp)
    assert abs(sum(fp) - f) <= 8 * EPS * sum(abs(v) for v in fp)
    gsum, gmag = np.sum(gp, axis=0), np.sum(np.abs(gp), axis=0)
    assert (np.abs(gsum - grad) <= 8 * EPS * gmag + 1e-12 * np.abs(grad)).all()


@pytest.mark.gpu
def test_batch_accepts_contexts_with_the_goal():
    from mocohip.solver import HipBatch

    def study():
        st = configs.gait10dof18musc_inverse(2)
        comp = Bhargava2004Metabolics("metabolics", use_smoothing=True)
        comp.add_muscle("soleus_r", "/forceset/soleus_r")
        st.problem.model.add_component(comp)
        st.problem.goals = [MocoControlGoal("effort", 1.0),
                            MocoOutputGoal("met", 1.0, output_path="/metabolics|total_metabolic_rate")]
        return st
    nlps = [_hip(study()), _hip(study())]
    batch = HipBatch(nlps)
    batch.close()
    for n in nlps:
        n.close()


# ---- 13. known answer by solve, 14. analyze --------------------------------------

@pytest.fixture(scope="module")
def held():
    """The held-mass study, its NLP and its solution, once for the module."""
    st = configs.hanging_muscle_metabolics(5, hold=0.15)
    nlp = st.create_nlp()
    try:
        yield st, nlp, st.solve(nlp=nlp)
    finally:
        nlp.close()


def _held_closed_form(st):
    """The held mass: speed 0 at every grid point, so the fibre velocity is 0,
    and m udot = m g - T = 0 fixes the tendon force at m g; the force is linear
    in the activation, which follows; adot = 0 then puts the excitation on the
    activation.  (a, Edot + basal rate, dE/da, dE/de, dT/da)."""
    ck = Checker(st)
    mu = st.problem.model.muscles[0]
    comp = st.problem.model.components[0]
    struct = ck.rep.compiled._muscles[0]
    T = lambda a: dict(zip(NAMES, restated_outputs(struct, 0.15, 0.0, a, a, 0.0, 0.0)))["tendon_force"]   # noqa: E731
    mg = configs.HANGING_MUSCLE_MASS * configs.HANGING_MUSCLE_GRAVITY
    dTda = T(1.0) - T(0.0)
    a = (mg - T(0.0)) / dTda
    assert 0.0 < a < 1.0 and abs(T(a) - mg) <= 1e-12

    def E(act, exc):
        q = dict(zip(NAMES, restated_outputs(struct, 0.15, 0.0, act, exc, 0.0, 0.0)))
        mp = comp.muscles[0]
        return ref.muscle_rates(comp, mp, ref.muscle_mass(mp, mu), mu.max_isometric_force, q)["total"] \
            + ref.basal_rate(comp, st.problem.model)
    d = 1e-6
    out = a, E(a, a), (E(a + d, a) - E(a - d, a)) / (2 * d), (E(a, a + d) - E(a, a - d)) / (2 * d), dTda
    ck.orc.close()
    return out


@pytest.mark.gpu
def test_the_held_mass_burns_the_closed_form_rate(held):
    """hanging_muscle_metabolics(5, hold=0.15), the goal on total_metabolic_rate
    over T = 0.5 s: f = T E with E = Edot(a, e = a) + the basal rate from
    _held_closed_form (the steady point: it is feasible, so f <= T E up to the
    value margin).  From below, to first order in the constraints' slack: the
    quadrature of the N = 5 speed defects is that of m g - T(a_k) over m, as in
    test_the_held_mass_weighs_m_g, and the tendon force is linear in the
    activation, so with the solver's constraint tolerance c = 1e-8 and its
    relaxation of the two speed bounds by at most 1e-8 each
        |sum quad_k (a_k - a)| <= m (N c + 2e-8) / |dT/da| = da;
    the activation defects hold the quadrature of adot = rate (e_k - a_k) to
    N c, and rate >= 1 / (4 tau_d) (half the deactivation rate at its
    slowest), so |sum quad_k (e_k - a)| <= da + 4 tau_d N c = de, and
        |f - T E| <= |dE/da| da + |dE/de| de + T 1e-10 (|E| + 1).
    The constraints alone do not exclude an excitation that varies over the
    mesh; the bound holds for the steady point the solver converges to from the
    bounds' midpoints, and the measured difference is printed."""
    st, nlp, sol = held
    assert sol.stats.success, sol.stats.status
    T, N = 0.5, 5
    a, E, dEda, dEde, dTda = _held_closed_form(st)
    ctol = st.solver.optim_constraint_tolerance if st.solver.optim_constraint_tolerance > 0 else 1e-8
    da = configs.HANGING_MUSCLE_MASS * (N * ctol + 2e-8) / abs(dTda)
    de = da + 4.0 * st.problem.model.muscles[0].deactivation_time_constant * N * ctol
    bound = abs(dEda) * da + abs(dEde) * de + T * TOL * (abs(E) + 1.0)
    f = float(sol.stats.objective)
    print("held mass: a =", a, "E =", E, "f - T E =", f - T * E, "bound", bound)
    assert abs(f - T * E) <= bound, (f, T * E, bound)


@pytest.mark.gpu
def test_analyze_columns_values_and_sto_round_trip(tmp_path, held):
    st, nlp, sol = held
    tab = st.analyze(sol, [r"/metabolics\|.*", r".*\|activation"], nlp=nlp)
    cols = ["/forceset/actuator|activation"] + ["/metabolics|" + o for o in OUT[:-1]] + \
        ["/metabolics|muscle_metabolic_rate:/forceset/actuator"]
    assert list(tab.columns) == cols   # the muscle's columns first
    x = sol.to_iterate(nlp)
    rows = _grid_rows(nlp, x)
    want = nlp.eval_metabolics(st.problem.model.components[0], rows)
    assert np.array_equal(np.asarray(tab.times), rows[:, 0])
    for k, c in enumerate(cols[1:]):
        assert np.array_equal(tab.columns[c], want[:, k]), c
    path = tmp_path / "outputs.sto"
    write_table(tab, str(path))
    back = read_table(str(path))
    assert list(back.columns) == cols and np.array_equal(back.times, tab.times)
    for c in cols:
        assert np.array_equal(back.columns[c], tab.columns[c])
    assert list(st.analyze(sol, [".*total_shortening_rate"], nlp=nlp).columns) == ["/metabolics|total_shortening_rate"]
    assert list(st.analyze(sol, [".*muscle_metabolic_rate:.*actuator"], nlp=nlp).columns) == [cols[-1]]
    assert list(st.analyze(sol, ["nothing"], nlp=nlp).columns) == []
