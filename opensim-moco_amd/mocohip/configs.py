"""The BASELINE.json configurations as MocoStudy builders.

  sliding_mass        configs[0]: exampleSlidingMass (Moco/Examples/C++/
                      exampleSlidingMass/exampleSlidingMass.cpp:35-90)
  double_pendulum     configs[1]: ModelFactory::createNLinkPendulum(2)
                      (Moco/Moco/Components/ModelFactory.cpp:33-89) with the
                      bounds of testImplicit.cpp:63-75
  gait10dof18musc     configs[2]: MocoTrack gait10dof18musc
                      (Moco/Tests/testMocoTrack.cpp:46-68) with the muscles
                      replaced by DeGrooteFregly2016Muscle
                      (ModOpReplaceMusclesWithDeGrooteFregly2016) instead of
                      removed, plus ModOpAddReserves(100) and the GRF
                      ExternalLoads; MocoTrack settings from MocoTrack.cpp:54-132.
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional

import numpy as np

from .model import (Axis, Body, Coordinate, CoordinateActuator, DataTable,
                    ExternalForce, Function, Joint, Marker, Model, SpringGeneralizedForce, model_from_dict)
from . import abi
from .osim import add_reserves
from .problem import (Constant, GCVSpline, ImplicitAuxiliaryDerivativesTerm,
                      MocoControlBoundConstraint, MocoControlGoal, MocoFrameDistanceConstraint,
                      MocoAccelerationTrackingGoal, MocoInitialActivationGoal, MocoJointReactionGoal,
                      FrameReference, MocoAngularVelocityTrackingGoal, MocoFinalTimeGoal, MocoMarkerFinalGoal, MocoMarkerTrackingGoal,
                      MarkersReference, MocoOrientationTrackingGoal, MocoOutputGoal, MocoProblem, MocoStateTrackingGoal,
                      MocoTranslationTrackingGoal, PiecewiseLinearFunction)
from .solver import MocoHipSolver, MocoStudy

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def sliding_mass(num_mesh_intervals: int = 50, dynamics: str = "explicit") -> MocoStudy:
    m = Model("sliding_mass", gravity=(0, 0, 0))
    m.add_body(Body("body", 2.0, (0, 0, 0), (0, 0, 0, 0, 0, 0)))
    pos = Coordinate("position", (-math.inf, math.inf), "translational", path="/slider/position")
    m.add_joint(Joint.slider("slider", "ground", "body", pos))
    m.add_coordinate_actuator(CoordinateActuator("actuator", "position", 1.0, path="/actuator"))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, (0.0, 5.0))
    p.set_state_info("/slider/position/value", (-5, 5), 0, 1)
    p.set_state_info("/slider/position/speed", (-50, 50), 0, 0)
    p.set_control_info("/actuator", (-50, 50))
    p.add_goal(MocoFinalTimeGoal())
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


# testMocoParameters.cpp:34-37: the oscillator's true mass and stiffness
OSCILLATOR_STIFFNESS = 100.0
OSCILLATOR_MASS = 5.0
OSCILLATOR_FINAL_TIME = math.pi * math.sqrt(OSCILLATOR_MASS / OSCILLATOR_STIFFNESS)


def _oscillator(body_mass: float, springs) -> Model:
    """createOscillatorModel / createOscillatorTwoSpringsModel
    (testMocoParameters.cpp:38-58,103-133): a body on a SliderJoint
    ("slider", coordinate "position"), no gravity, SpringGeneralizedForce(s)
    on the coordinate, rest length 0, no viscosity; a marker at the body's
    origin stands for the test's FinalPositionGoal (below)."""
    m = Model("oscillator", gravity=(0, 0, 0))
    m.add_body(Body("body", body_mass, (0, 0, 0), (0, 0, 0, 0, 0, 0)))
    pos = Coordinate("position", (-math.inf, math.inf), "translational", path="/slider/position")
    m.add_joint(Joint.slider("slider", "ground", "body", pos))
    for name, k in springs:
        m.add_spring(SpringGeneralizedForce(name, "position", stiffness=k, rest_length=0.0, viscosity=0.0))
    m.add_marker(Marker("body_origin", "body", (0.0, 0.0, 0.0)))
    return m


def _oscillator_study(m: Model, num_mesh_intervals: int) -> MocoStudy:
    """The test's problem (testMocoParameters.cpp:81-94,141-156): time in [0,
    pi sqrt(MASS / STIFFNESS)], position starting at -0.5 and ending in [0.25,
    0.75], speed 0 at both ends, and FinalPositionGoal -- (final position -
    0.5)^2 (:60-72), here MocoMarkerFinalGoal of the body origin against (0.5,
    0, 0): the same cost, since the origin is at (q, 0, 0)."""
    p = MocoProblem(m)
    p.set_time_bounds(0, OSCILLATOR_FINAL_TIME)
    p.set_state_info("/slider/position/value", (-5.0, 5.0), -0.5, (0.25, 0.75))
    p.set_state_info("/slider/position/speed", (-20, 20), 0, 0)
    p.add_goal(MocoMarkerFinalGoal(name="final_position", point_name="/markerset/body_origin",
                                   reference_location=(0.5, 0.0, 0.0)))
    return MocoStudy(p, MocoHipSolver(num_mesh_intervals=num_mesh_intervals))


def oscillator_mass(num_mesh_intervals: int = 25) -> MocoStudy:
    """testMocoParameters.cpp:78-99 ("Oscillator mass"): the body starts at
    half the true mass; MocoParameter "oscillator_mass" writes the body's
    mass, bounds [0, 10]; the solve must recover MASS within 0.3 %."""
    st = _oscillator_study(_oscillator(0.5 * OSCILLATOR_MASS, [("spring", OSCILLATOR_STIFFNESS)]),
                           num_mesh_intervals)
    st.problem.add_parameter("oscillator_mass", "body", "mass", (0, 10))
    return st


def oscillator_two_springs(num_mesh_intervals: int = 25) -> MocoStudy:
    """testMocoParameters.cpp:135-166 ("One parameter two springs"): two
    springs of a quarter of the stiffness each, ONE MocoParameter
    "spring_stiffness" writing both (bounds [0, 100]); the solve must find
    half the stiffness within 0.3 %."""
    st = _oscillator_study(_oscillator(OSCILLATOR_MASS, [("spring1", 0.25 * OSCILLATOR_STIFFNESS),
                                                         ("spring2", 0.25 * OSCILLATOR_STIFFNESS)]),
                           num_mesh_intervals)
    st.problem.add_parameter("spring_stiffness", ["spring1", "spring2"], "stiffness", (0, 100))
    return st


def gait10dof18musc_parameters(num_mesh_intervals: int = 6, **kw) -> MocoStudy:
    """gait10dof18musc with MocoParameters over every property kind a
    muscle-driven gait model offers (MocoParameter.h:91-170; test case, no
    reference counterpart on this model): one parameter on both femurs'
    mass, both soleus' max_isometric_force, the torso's mass-center y (a
    vector-property element), a reserve actuator's optimal_force."""
    st = gait10dof18musc(num_mesh_intervals, **kw)
    p = st.problem
    p.add_parameter("femur_mass", ["/bodyset/femur_r", "/bodyset/femur_l"], "mass", (5.0, 12.0))
    p.add_parameter("soleus_fmax", ["/forceset/soleus_r", "/forceset/soleus_l"], "max_isometric_force",
                    (2000.0, 5000.0))
    p.add_parameter("torso_com_y", "/bodyset/torso", "mass_center", (0.25, 0.45), property_element=1)
    p.add_parameter("pelvis_tilt_reserve", "/forceset/reserve_jointset_ground_pelvis_pelvis_tilt",
                    "optimal_force", (1.0, 50.0))
    return st


def sliding_mass_interface(num_mesh_intervals: int = 19, scheme: str = "trapezoidal",
                           dynamics: str = "explicit") -> MocoStudy:
    """testMocoInterface.cpp:41-83 ("Sliding mass", :1701-1742): a 10 kg
    mass on a slider, control in [-10, 10] N, from x = 0 to x = 1 at rest,
    minimum final time in [0, 10], trapezoidal, 19 mesh intervals; the
    reference's solution is bang-bang with final time 2.0."""
    m = Model("sliding_mass", gravity=(0, 0, 0))
    m.add_body(Body("body", 10.0, (0, 0, 0), (0, 0, 0, 0, 0, 0)))
    pos = Coordinate("position", (-math.inf, math.inf), "translational", path="/slider/position")
    m.add_joint(Joint.slider("slider", "ground", "body", pos))
    m.add_coordinate_actuator(CoordinateActuator("actuator", "position", 1.0, -10.0, 10.0,
                                                 path="/actuator"))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, (0.0, 10.0))
    p.set_state_info("/slider/position/value", (0, 1), 0, 1)
    p.set_state_info("/slider/position/speed", (-100, 100), 0, 0)
    p.add_goal(MocoFinalTimeGoal())
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics, enforce_constraint_derivatives=False)
    return MocoStudy(p, s)


def n_link_pendulum(num_links: int, inertia=(1, 1, 1, 0, 0, 0)) -> Model:
    """ModelFactory::createNLinkPendulum (inertia=(0,)*6: point masses at
    the link tips, tropter's double pendulum, test_double_pendulum.cpp:45-74)."""
    m = Model({1: "pendulum", 2: "double_pendulum"}.get(num_links, f"{num_links}_link_pendulum"))
    prev = "ground"
    for i in range(num_links):
        m.add_body(Body(f"b{i}", 1.0, (0, 0, 0), tuple(inertia)))
        q = Coordinate(f"q{i}", (-math.pi / 2, math.pi / 2))
        m.add_joint(Joint.pin(f"j{i}", prev, f"b{i}", q, loc_in_child=(-1, 0, 0)))
        prev = f"b{i}"
    for i in range(num_links):
        m.add_coordinate_actuator(CoordinateActuator(f"tau{i}", f"q{i}", 1.0, path=f"/tau{i}"))
    for i in range(num_links):   # ModelFactory.cpp:74-75: at each body's origin
        m.add_marker(Marker(f"marker{i}", f"b{i}", (0.0, 0.0, 0.0)))
    return m


def double_pendulum(num_mesh_intervals: int = 100, scheme: str = "hermite-simpson",
                    dynamics: str = "explicit") -> MocoStudy:
    """testImplicit.cpp:63-75 solves this problem in both dynamics modes."""
    m = n_link_pendulum(2)
    p = MocoProblem(m)
    p.set_time_bounds(0.0, (0.0, 5.0))
    p.set_state_info("/jointset/j0/q0/value", (-10, 10), 0)
    p.set_state_info("/jointset/j0/q0/speed", (-50, 50), 0, 0)
    p.set_state_info("/jointset/j1/q1/value", (-10, 10), 0)
    p.set_state_info("/jointset/j1/q1/speed", (-50, 50), 0, 0)
    p.set_control_info("/tau0", (-100, 100))
    p.set_control_info("/tau1", (-100, 100))
    p.add_goal(MocoFinalTimeGoal(weight=0.001))
    p.add_goal(MocoControlGoal(weight=1e-3))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def double_pendulum_coupled(num_mesh_intervals: int = 20, scheme: str = "hermite-simpson",
                           dynamics: str = "explicit", enforce_constraint_derivatives: bool = True,
                           coupler: str = "linear", minimize_multipliers: bool = True) -> MocoStudy:
    """testConstraints.cpp:620-690 (testDoublePendulumCoordinateCoupler): a
    CoordinateCouplerConstraint q1 = -2 q0 + pi (LinearFunction(-2, pi)),
    control goal, HS N=20, both dynamics modes, with and without enforcing
    the constraint derivatives, minimizing the Lagrange multipliers with
    weight 10.  coupler="spline":
    the same constraint through a SimmSpline of the linear relation plus a
    quadratic term, so that f'' != 0 (acceleration errors and the
    velocity-correction Jacobian see the curvature)."""
    from .model import CoordinateCouplerConstraint, Function
    m = n_link_pendulum(2)
    if coupler == "linear":
        f = Function.linear("q0", -2.0, math.pi)
    else:
        xs = np.linspace(-6.0, 6.0, 13)
        f = Function.simm_spline("q0", xs, -2.0 * xs + math.pi + 0.1 * xs * xs)
    m.add_constraint(CoordinateCouplerConstraint("q0_q1_coupler", "q1", f))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, 1.0)
    p.set_state_info("/jointset/j0/q0/value", (-5, 5), 0, math.pi / 2)
    p.set_state_info("/jointset/j0/q0/speed", (-10, 10), 0, 0)
    p.set_state_info("/jointset/j1/q1/value", (-10, 10))
    p.set_state_info("/jointset/j1/q1/speed", (-5, 5), 0, 0)
    p.set_control_info("/tau0", (-50, 50))
    p.set_control_info("/tau1", (-50, 50))
    p.add_goal(MocoControlGoal())
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics,
                      enforce_constraint_derivatives=enforce_constraint_derivatives,
                      minimize_lagrange_multipliers=minimize_multipliers, lagrange_multiplier_weight=10.0)
    return MocoStudy(p, s)


def double_pendulum_swingup(num_mesh_intervals: int = 29, scheme: str = "trapezoidal",
                            dynamics: str = "explicit", point_masses: bool = False) -> MocoStudy:
    """testImplicit.cpp:30-100 (solveDoublePendulumSwingup): final-time goal
    (weight 0.001) + MocoMarkerFinalGoal on /markerset/marker1 to (0, 2, 0)
    (weight 1000), trapezoidal, N=29, both dynamics modes.  point_masses:
    tropter's pendulum (no link inertia; test_double_pendulum.cpp:80-150)."""
    m = n_link_pendulum(2, inertia=(0, 0, 0, 0, 0, 0) if point_masses else (1, 1, 1, 0, 0, 0))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, (0.0, 5.0))
    p.set_state_info("/jointset/j0/q0/value", (-10, 10), 0)
    p.set_state_info("/jointset/j0/q0/speed", (-50, 50), 0, 0)
    p.set_state_info("/jointset/j1/q1/value", (-10, 10), 0)
    p.set_state_info("/jointset/j1/q1/speed", (-50, 50), 0, 0)
    p.set_control_info("/tau0", (-100, 100))
    p.set_control_info("/tau1", (-100, 100))
    p.add_goal(MocoFinalTimeGoal(weight=0.001))
    p.add_goal(MocoMarkerFinalGoal("final", weight=1000.0, point_name="/markerset/marker1",
                                   reference_location=(0.0, 2.0, 0.0)))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def pendulum_control_bound(num_mesh_intervals: int = 20, section: str = "lower",
                           scheme: str = "hermite-simpson",
                           dynamics: str = "explicit") -> MocoStudy:
    """The MocoControlBoundConstraint problems of testConstraints.cpp:1460-1540
    (ModelFactory::createPendulum): "lower" (Constant 0.1318 lower bound),
    "upper" (Constant 11.236 upper bound, free final time), "equality"
    (PiecewiseLinearFunction lower bound with equality_with_lower), and
    "both" (GCVSpline lower and Constant upper bound, two equations)."""
    m = n_link_pendulum(1)
    p = MocoProblem(m)
    c = p.add_path_constraint(MocoControlBoundConstraint())
    c.add_control_path("/tau0")
    if section == "upper":
        p.set_time_bounds(0.0, (0.1, 10.0))
        p.set_state_info("/jointset/j0/q0/value", (0, 1), 0, 0.53)
        p.set_state_info("/jointset/j0/q0/speed", (-10, 10), 0, 0)
        p.set_control_info("/tau0", (-20, 20))
        p.add_goal(MocoFinalTimeGoal())
        c.set_upper_bound(Constant(11.236))
    else:
        p.set_time_bounds(0.0, 1.0)
        p.set_state_info("/jointset/j0/q0/value", (-10, 10), 0)
        p.set_state_info("/jointset/j0/q0/speed", (-10, 10), 0)
        p.set_control_info("/tau0", (-5, 5))
        p.add_goal(MocoControlGoal())
        if section == "lower":
            c.set_lower_bound(Constant(0.1318))
        elif section == "equality":
            c.set_lower_bound(PiecewiseLinearFunction([0, 0.2, 0.7, 1], [0, 0.5316, -0.3137, 0.0319]))
            c.set_equality_with_lower(True)
        elif section == "both":
            c.set_lower_bound(GCVSpline(5, [0, 0.2, 0.45, 0.7, 0.85, 1.0],
                                        [-0.4, 0.1, -0.2, 0.3, 0.0, -0.1]))
            c.set_upper_bound(Constant(2.5))
        else:
            raise ValueError(section)
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def _load(name):
    with open(os.path.join(DATA, name)) as fh:
        return json.load(fh)


def gait10dof18musc_model(muscles: bool = True, tendon_compliance: bool = False,
                          reserves: float = 100.0, external_loads: bool = True,
                          tendon_dynamics: str = "explicit") -> Model:
    """tendon_dynamics: DeGrooteFregly2016Muscle tendon_compliance_dynamics_mode
    of the compliant tendons ("implicit": the MocoInverse test setting,
    ModOpTendonComplianceDynamicsModeDGF("implicit"), testMocoInverse.cpp:127)."""
    m = model_from_dict(_load("gait10dof18musc.json"))
    if not muscles:
        m.actuators = [a for a in m.actuators if not hasattr(a, "points")]
        m.muscles = []
    for mu in m.muscles:
        mu.ignore_tendon_compliance = not tendon_compliance
        mu.tendon_compliance_dynamics_mode = tendon_dynamics
    if reserves:
        add_reserves(m, reserves)
    if external_loads:
        grf = _load("walk_gait1018_subject01_grf.json")
        cols = {k: np.asarray(v) for k, v in grf["columns"].items()}
        m.add_table(DataTable("grf", np.asarray(grf["time"]), cols, degree=3))
        for ef in grf["external_forces"]:
            if ef["force_expressed_in_body"] != "ground" or ef["point_expressed_in_body"] != "ground":
                raise NotImplementedError("ExternalForce must be expressed in ground")
            m.add_external_force(ExternalForce(ef["name"], ef["body"], "grf",
                                               ef["force_identifier"], ef["point_identifier"],
                                               ef["torque_identifier"]))
    return m


def gait10dof18musc(num_mesh_intervals: int = 200, muscles: bool = True,
                    tendon_compliance: bool = False,
                    fd_scheme: str = "forward", dynamics: str = "explicit",
                    control_bounds: bool = False, tendon_dynamics: str = "explicit") -> MocoStudy:
    """MocoTrack gait10dof18musc (config 3).  MocoTrack: states tracking goal
    (weight 1, GCVSpline reference), control effort goal (0.001), time
    [0.01, 1.3], explicit dynamics, forward FD (MocoTrack.cpp:54-132).
    control_bounds: adds a MocoControlBoundConstraint on the soleus and
    tibialis anterior excitations (GCVSpline lower, Constant upper bound) and
    one on the hip flexor reserve (Constant upper bound) as path constraints
    (not part of the reference MocoTrack setup)."""
    m = gait10dof18musc_model(muscles=muscles, tendon_compliance=tendon_compliance,
                              tendon_dynamics=tendon_dynamics)
    ref = _load("walk_gait1018_state_reference.json")
    cols = {k: np.asarray(v) for k, v in ref["columns"].items()}
    m.add_table(DataTable("state_reference", np.asarray(ref["time"]), cols, degree=5))
    p = MocoProblem(m)
    p.add_goal(MocoStateTrackingGoal("state_tracking", 1.0, DataTable(
        "state_reference", np.asarray(ref["time"]), cols, degree=5)))
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    p.set_time_bounds(0.01, 1.3)
    if control_bounds:
        names = m.control_names()
        picks = [n for n in names if n.endswith(("soleus_r", "tib_ant_r"))] if muscles else []
        c = p.add_path_constraint(MocoControlBoundConstraint("excitation_band"))
        for n in picks:
            c.add_control_path(n)
        c.set_lower_bound(GCVSpline(5, np.linspace(0.0, 1.4, 8),
                                    0.02 + 0.01 * np.sin(np.linspace(0.0, 3.0, 8))))
        c.set_upper_bound(Constant(0.9))
        r = p.add_path_constraint(MocoControlBoundConstraint("reserve_cap"))
        r.add_control_path(names[-1])
        r.set_upper_bound(Constant(0.5))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals,
                      optim_finite_difference_scheme=fd_scheme, multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def gait10dof18musc_feet_apart(num_mesh_intervals: int = 200, projection: str = "none",
                               **kw) -> MocoStudy:
    """The gait10dof18musc study plus a MocoFrameDistanceConstraint that keeps
    the feet apart: one pair of offset frames on calcn_r and calcn_l, at least
    0.1 m apart ("vector" / "plane": along / normal to the medio-lateral
    direction, slightly tilted so that no component of it is zero)."""
    st = gait10dof18musc(num_mesh_intervals, **kw)
    m = st.problem.model
    m.add_offset_frame("mid_foot_r", "calcn_r", (0.1, 0.02, 0.01))
    m.add_offset_frame("mid_foot_l", "calcn_l", (0.1, 0.02, -0.01))
    c = st.problem.add_path_constraint(MocoFrameDistanceConstraint("feet_apart"))
    c.add_frame_pair("/bodyset/calcn_r/mid_foot_r", "/bodyset/calcn_l/mid_foot_l", 0.1, math.inf)
    c.set_projection(projection)
    if projection != "none":
        c.set_projection_vector((0.1, 0.2, 1.0))
    return st


def gimbal_frame_distance(num_mesh_intervals: int = 25, dynamics: str = "explicit",
                          scheme: str = "hermite-simpson", fd_scheme: str = "forward") -> MocoStudy:
    """testConstraints.cpp:1591-1658 (MocoFrameDistanceConstraint): a body of
    mass 1, inertia 1 on a GimbalJoint at (0, 1, 0) of ground (parent
    orientation (0, 0, -pi/2), child location (-1, 0, 0)), reserves of optimal
    force 50 on qx, qy, qz (ModOpAddReserves(50)), time [0, 0.5], the state
    infos of :1626-1632, the pair /ground - /bodyset/body at least 0.1 apart,
    and a MocoMarkerFinalGoal of the body origin to (0, 0.292893, 0.707107).
    At q = 0 the body origin is the ground origin, so the straight path of qy
    from pi/4 to -pi/4 violates the constraint -- and there the constraint's
    gradient vanishes.  fd_scheme: forward differences by default, a deviation
    from the reference's solver default (central): from the bounds guess the
    interior-point restatement (mocohip.ipm) ends in Restoration_Failed with
    central differences (frame-distance constraints)."""
    m = Model("gimbal_pendulum")
    m.add_body(Body("body", 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
    qx, qy, qz = (Coordinate(n, (-math.inf, math.inf)) for n in ("qx", "qy", "qz"))
    m.add_joint(Joint.gimbal("gimbal", "ground", "body", qx, qy, qz, loc_in_parent=(0, 1, 0),
                             orient_in_parent=(0, 0, -math.pi / 2), loc_in_child=(-1, 0, 0)))
    m.add_marker(Marker("marker", "body", (0.0, 0.0, 0.0)))
    m.add_offset_frame("body_center", "body", (-0.5, 0.0, 0.0))
    add_reserves(m, 50.0)
    p = MocoProblem(m)
    p.set_time_bounds(0, 0.5)
    third = math.pi / 3
    p.set_state_info("/jointset/gimbal/qx/value", (-third, third), 0)
    p.set_state_info("/jointset/gimbal/qy/value", (-third, third), math.pi / 4, -math.pi / 4)
    p.set_state_info("/jointset/gimbal/qz/value", (-third, third), 0)
    for n in ("qx", "qy", "qz"):
        p.set_state_info(f"/jointset/gimbal/{n}/speed", (-10, 10), 0, 0)
    c = p.add_path_constraint(MocoFrameDistanceConstraint())
    c.add_frame_pair("/ground", "/bodyset/body", 0.1, math.inf)
    p.add_goal(MocoMarkerFinalGoal("final_marker", point_name="/markerset/marker",
                                   reference_location=(0.0, 0.292893, 0.707107)))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics, optim_finite_difference_scheme=fd_scheme)
    return MocoStudy(p, s)


def double_pendulum_marker_tracking(num_mesh_intervals: int = 50, scheme: str = "hermite-simpson",
                                    fd_scheme: str = "central") -> MocoStudy:
    """exampleMarkerTracking.cpp:27-157: two links of mass 1 and inertia 1 on
    pin joints (coordinates in [-10, 10], child frames at (-1, 0, 0)), torque
    actuators with controls in [-40, 40], markers m0 / m1 at the body origins,
    time [0, 1], and one MocoMarkerTrackingGoal whose reference rows at t = 0,
    0.01, ..., 0.99 are the markers' locations for q0 = t pi / 2, q1 = t pi /
    4, with marker weights 100 and 10; 50 mesh intervals, the solver's
    defaults otherwise (Hermite-Simpson, central differences).  The example
    solves with the exact Hessian (:147); this path has the limited-memory
    approximation only, and with Ipopt's default memory of 6 pairs the
    interior-point restatement crawls (no scheme converges within 3000
    iterations), so the config keeps 100 pairs (marker
    tracking)."""
    m = Model("double_pendulum")
    prev = "ground"
    for i in range(2):
        m.add_body(Body(f"b{i}", 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
        m.add_joint(Joint.pin(f"j{i}", prev, f"b{i}", Coordinate(f"q{i}", (-10, 10)), loc_in_child=(-1, 0, 0)))
        prev = f"b{i}"
    for i in range(2):
        m.add_coordinate_actuator(CoordinateActuator(f"tau{i}", f"q{i}", 1.0, -40.0, 40.0, path=f"/tau{i}"))
    for i in range(2):
        m.add_marker(Marker(f"m{i}", f"b{i}", (0.0, 0.0, 0.0)))
    times, rows = [], []
    t = 0.0
    while t < 1.0:   # for (double time = 0; time < finalTime; time += 0.01)
        q0, q1 = (t / 1.0) * 0.5 * math.pi, (t / 1.0) * 0.25 * math.pi
        m0 = (math.cos(q0), math.sin(q0), 0.0)
        rows.append([m0, (m0[0] + math.cos(q0 + q1), m0[1] + math.sin(q0 + q1), 0.0)])
        times.append(t)
        t += 0.01
    ref = MarkersReference("markers_reference", np.asarray(times), ["/markerset/m0", "/markerset/m1"],
                           np.asarray(rows), {"/markerset/m0": 100.0, "/markerset/m1": 10.0})
    m.add_table(ref.flatten())
    p = MocoProblem(m)
    p.set_time_bounds(0, 1.0)
    p.add_goal(MocoMarkerTrackingGoal("marker_tracking", 1.0, ref))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme, optim_ipopt_limited_memory_max_history=100)
    return MocoStudy(p, s)


# The markers of the gait10dof18musc marker-tracking configs: (name, body,
# location in the body frame, m).  The model data has none; these sit where a
# gait marker set puts them (pelvis: the anterior and posterior superior iliac
# spines' midpoints; thigh and shank: mid-segment, on the anterior / lateral
# surface; the knee and ankle joint lines; heel and toe), at offsets rounded
# from the segment geometry of the gait2392 family this model belongs to.
GAIT_MARKERS = (
    ("pelvis_front", "pelvis", (0.02, 0.03, 0.0)),
    ("pelvis_back", "pelvis", (-0.15, 0.04, 0.0)),
    ("thigh_r", "femur_r", (0.05, -0.2, 0.06)),
    ("knee_r", "femur_r", (0.0, -0.4, 0.05)),
    ("shank_r", "tibia_r", (0.03, -0.2, 0.05)),
    ("ankle_r", "tibia_r", (-0.01, -0.4, 0.05)),
    ("heel_r", "calcn_r", (-0.02, 0.02, 0.0)),
    ("toe_r", "toes_r", (0.03, 0.01, 0.0)),
    ("thigh_l", "femur_l", (0.05, -0.2, -0.06)),
    ("knee_l", "femur_l", (0.0, -0.4, -0.05)),
    ("shank_l", "tibia_l", (0.03, -0.2, -0.05)),
    ("ankle_l", "tibia_l", (-0.01, -0.4, -0.05)),
    ("heel_l", "calcn_l", (-0.02, 0.02, 0.0)),
    ("toe_l", "toes_l", (0.03, 0.01, 0.0)),
)


def synthesize_markers_reference(m: Model, times, coordinate_columns,
                                 name: str = "markers_reference") -> MarkersReference:
    """The model's markers' trajectories (Model.marker_locations_in_ground)
    along coordinate trajectories given by coordinate value path, as a
    MarkersReference labelled by marker name."""
    bypath = {c.path + "/value": c.name for c in m.coordinates()}
    cols = {bypath[k]: np.asarray(v, float) for k, v in coordinate_columns.items() if k in bypath}
    byname = {mk.name: path for path, mk in m.markers.items()}
    labels = list(byname)
    pos = np.empty((len(times), len(labels), 3))
    for r in range(len(times)):
        loc = m.marker_locations_in_ground({n: v[r] for n, v in cols.items()})
        for i, n in enumerate(labels):
            pos[r, i] = loc[byname[n]]
    return MarkersReference(name, np.asarray(times, float), labels, pos)


def gait10dof18musc_marker_track(num_mesh_intervals: int = 200, muscles: bool = True,
                                 fd_scheme: str = "forward", dynamics: str = "explicit",
                                 markers=GAIT_MARKERS, ground_marker: bool = False) -> MocoStudy:
    """The gait10dof18musc study (configs[2]) in MocoTrack's marker mode
    (MocoTrack::configureMarkerTracking, MocoTrack.cpp:235-266): the
    state-tracking goal replaced by a MocoMarkerTrackingGoal "marker_tracking"
    (weight 1, every marker weight 1), the control-effort goal (0.001) kept,
    the time bounds the marker data's range, MocoTrack's solver settings.
    The markers are GAIT_MARKERS; their trajectories are synthesized from the
    bundled walking coordinate trajectories (walk_gait1018_state_reference) by
    forward kinematics, at the data's own rows.  No marker sits on the torso,
    so lumbar_extension drives none.  ``markers`` / ``ground_marker``: the
    few-marker variant the tests use (a marker fixed in ground, tracked
    against a reference that moves)."""
    m = gait10dof18musc_model(muscles=muscles)
    for name, body, loc in markers:
        m.add_marker(Marker(name, body, loc))
    data = _load("walk_gait1018_state_reference.json")
    times = np.asarray(data["time"])
    ref = synthesize_markers_reference(m, times, data["columns"])
    if ground_marker:
        m.add_marker(Marker("lab", "ground", (0.3, 0.1, -0.2)))
        ref.labels.append("lab")
        drift = np.stack([0.3 + 0.05 * times, 0.1 + 0.02 * np.sin(times), -0.2 + 0.0 * times], 1)
        ref.positions = np.concatenate([ref.positions, drift[:, None, :]], 1)
    m.add_table(ref.flatten())
    p = MocoProblem(m)
    p.add_goal(MocoMarkerTrackingGoal("marker_tracking", 1.0, ref))
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    p.set_time_bounds(float(times[0]), float(times[-1]))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, optim_finite_difference_scheme=fd_scheme,
                      multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


# gait10dof18musc_marker_track_few: pelvis, one femur, the opposite tibia, a
# foot; the tibia's and the foot's off the body origin
GAIT_MARKERS_FEW = (
    ("pelvis_origin", "pelvis", (0.0, 0.0, 0.0)),
    ("thigh_r", "femur_r", (0.0, 0.0, 0.0)),
    ("shank_l", "tibia_l", (0.03, -0.2, -0.05)),
    ("heel_r", "calcn_r", (-0.02, 0.02, 0.0)),
)


def gait10dof18musc_marker_track_few(num_mesh_intervals: int = 3, **kw) -> MocoStudy:
    """gait10dof18musc_marker_track with four markers (pelvis, femur_r,
    tibia_l, calcn_r) and one fixed in ground: small enough for N = 2-4, with
    a coordinate that drives no tracked marker (lumbar_extension)."""
    return gait10dof18musc_marker_track(num_mesh_intervals, markers=GAIT_MARKERS_FEW, ground_marker=True, **kw)


def double_pendulum_effort(num_mesh_intervals: int = 20, scheme: str = "hermite-simpson",
                           effort_weight: float = 1.0) -> MocoStudy:
    """testMocoGoals.cpp:209-232 (setupMocoStudyDoublePendulumMinimizeEffort):
    ModelFactory::createNLinkPendulum(2), a MocoControlGoal "effort", time [0,
    2], controls in [-100, 100], q0 from 0 to pi / 2, q1 from pi to 0, speeds
    in [-50, 50] from 0 to 0, 20 mesh intervals, convergence tolerance 1e-5,
    explicit dynamics."""
    m = n_link_pendulum(2)
    p = MocoProblem(m)
    p.add_goal(MocoControlGoal("effort", effort_weight))
    p.set_time_bounds(0, 2)
    p.set_control_info("/tau0", (-100, 100))
    p.set_control_info("/tau1", (-100, 100))
    p.set_state_info("/jointset/j0/q0/value", (-10, 10), 0, math.pi / 2)
    p.set_state_info("/jointset/j0/q0/speed", (-50, 50), 0, 0)
    p.set_state_info("/jointset/j1/q1/value", (-10, 10), math.pi, 0)
    p.set_state_info("/jointset/j1/q1/speed", (-50, 50), 0, 0)
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_convergence_tolerance=1e-5, multibody_dynamics_mode="explicit")
    return MocoStudy(p, s)


def states_table(trajectory, name: str = "states_reference") -> DataTable:
    """MocoTrajectory::exportToStatesTable: the states by path."""
    return DataTable(name, np.asarray(trajectory.time, float),
                     {n: np.ascontiguousarray(trajectory.states[:, i]) for i, n in enumerate(trajectory.state_names)})


def double_pendulum_swing_states(num_rows: int = 41) -> DataTable:
    """A smooth stand-in for the effort solution where none has been solved
    (tests of the lowering and of the kernel): q0 from 0 to pi / 2 and q1 from
    pi to 0 over [0, 2] along s(t) = (1 - cos(pi t / 2)) / 2, with the speeds
    that go with it."""
    t = np.linspace(0.0, 2.0, num_rows)
    sm, ds = 0.5 * (1.0 - np.cos(0.5 * math.pi * t)), 0.25 * math.pi * np.sin(0.5 * math.pi * t)
    return DataTable("states_reference", t, {
        "/jointset/j0/q0/value": 0.5 * math.pi * sm, "/jointset/j0/q0/speed": 0.5 * math.pi * ds,
        "/jointset/j1/q1/value": math.pi * (1.0 - sm), "/jointset/j1/q1/speed": -math.pi * ds})


def double_pendulum_frame_tracking(kind: str = "orientation", reference_solution=None,
                                   num_mesh_intervals: int = 20, scheme: str = "hermite-simpson",
                                   fd_scheme: str = "central") -> MocoStudy:
    """testMocoGoals.cpp:234-256 (testDoublePendulumTracking): the effort
    problem with the effort goal's weight 0.001 and a tracking goal "tracking"
    of ``kind`` ("translation" / "orientation" / "angular_velocity"; the last:
    testMocoGoals.cpp:319-325) on the frames /bodyset/b0 and
    /bodyset/b1, its states reference the effort solution (a MocoTrajectory or
    a states DataTable; None: double_pendulum_swing_states)."""
    st = double_pendulum_effort(num_mesh_intervals, scheme, effort_weight=0.001)
    st.solver.optim_finite_difference_scheme = fd_scheme
    if reference_solution is None:
        reference_solution = double_pendulum_swing_states()
    elif not isinstance(reference_solution, DataTable):
        reference_solution = states_table(reference_solution)
    cls = {"translation": MocoTranslationTrackingGoal, "orientation": MocoOrientationTrackingGoal,
           "angular_velocity": MocoAngularVelocityTrackingGoal}[kind]
    g = cls("tracking", 1.0, states_reference=reference_solution, frame_paths=["/bodyset/b0", "/bodyset/b1"])
    st.problem.model.add_table(g.reference_table(st.problem.model))
    st.problem.add_goal(g)
    return st


def gimbal_motion(times):
    """A smooth 3-D motion of the gimbal's (qx, qy, qz), within its +-pi / 3."""
    t = np.asarray(times, float)
    return {"qx": 0.6 * np.sin(2.0 * t + 0.3), "qy": 0.7 * np.cos(3.0 * t), "qz": -0.5 + 0.8 * t}


def gimbal_motion_rates(times):
    """d/dt of gimbal_motion."""
    t = np.asarray(times, float)
    return {"qx": 1.2 * np.cos(2.0 * t + 0.3), "qy": -2.1 * np.sin(3.0 * t), "qz": 0.8 + 0.0 * t}


def gimbal_frame_tracking(num_mesh_intervals: int = 2, scheme: str = "hermite-simpson",
                          fd_scheme: str = "central", angular_velocity: bool = False) -> MocoStudy:
    """gimbal_frame_distance's model (a body on a GimbalJoint) with a rotated
    offset frame "sensor" on the body (translation (-0.5, 0.1, 0.2),
    orientation (0.4, -0.7, 1.1)): orientation tracking of the sensor (weight
    2) and of the body frame, translation tracking of the sensor (weight 3),
    the references given as tables computed along gimbal_motion at 26 rows,
    plus a control-effort goal (0.001).  ``angular_velocity``: also a
    MocoAngularVelocityTrackingGoal "angular_velocity_tracking" (weight 0.25)
    of the sensor (weight 1.5) after the other two, its reference the sensor's
    angular velocity along the same motion."""
    m = gimbal_frame_distance(num_mesh_intervals).problem.model
    m.add_offset_frame("sensor", "body", (-0.5, 0.1, 0.2), (0.4, -0.7, 1.1))
    sensor = "/bodyset/body/sensor"
    times = np.linspace(0.0, 0.5, 26)
    mot = gimbal_motion(times)
    poses = [[m.frame_pose_in_ground(f, {n: v[r] for n, v in mot.items()}) for f in (sensor, "/bodyset/body")]
             for r in range(len(times))]
    rot = FrameReference(times, [sensor, "/bodyset/body"], np.array([[ps[1] for ps in row] for row in poses]))
    pos = FrameReference(times, [sensor, "/bodyset/body"], np.array([[ps[0] for ps in row] for row in poses]))
    go = MocoOrientationTrackingGoal("orientation_tracking", 1.0, reference=rot, frame_weights={sensor: 2.0})
    gt = MocoTranslationTrackingGoal("translation_tracking", 0.5, reference=pos, frame_paths=[sensor],
                                     frame_weights={sensor: 3.0})
    p = MocoProblem(m)
    p.set_time_bounds(0, 0.5)
    third = math.pi / 3
    for n in ("qx", "qy", "qz"):
        p.set_state_info(f"/jointset/gimbal/{n}/value", (-third, third))
        p.set_state_info(f"/jointset/gimbal/{n}/speed", (-10, 10))
    goals = [go, gt]
    if angular_velocity:
        rate = gimbal_motion_rates(times)
        om = [[m.frame_angular_velocity_in_ground(sensor, {n: v[r] for n, v in mot.items()},
                                                  {n: v[r] for n, v in rate.items()})]
              for r in range(len(times))]
        goals.append(MocoAngularVelocityTrackingGoal("angular_velocity_tracking", 0.25,
                                                     reference=FrameReference(times, [sensor], np.array(om)),
                                                     frame_weights={sensor: 1.5}))
    for g in goals:
        m.add_table(g.reference_table(m))
        p.add_goal(g)
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme)
    return MocoStudy(p, s)


GAIT_ORIENTATION_FRAMES_FEW = ("/bodyset/pelvis", "/bodyset/femur_r", "/bodyset/femur_l", "/bodyset/tibia_r",
                               "/bodyset/tibia_l")
# gait10dof18musc_frame_track: the five above, and a sensor frame on each foot
GAIT_ORIENTATION_FRAMES = GAIT_ORIENTATION_FRAMES_FEW + ("/bodyset/calcn_r/imu_r", "/bodyset/calcn_l/imu_l")


def gait10dof18musc_frame_track(num_mesh_intervals: int = 200, markers=GAIT_MARKERS,
                                frames=GAIT_ORIENTATION_FRAMES, translation: bool = False,
                                **kw) -> MocoStudy:
    """gait10dof18musc_marker_track plus a MocoOrientationTrackingGoal
    "orientation_tracking" (weight 1, frame weights 1) on ``frames`` -- the
    segments an inertial-sensor set covers; the foot sensors are offset frames
    rotated in their bodies -- and, with ``translation``, a
    MocoTranslationTrackingGoal of the pelvis; the states reference is the
    bundled walking coordinate data, so the references are the frames' poses
    by forward kinematics at the data's rows.  Markers, segment orientations
    and the pelvis position share one kernel launch."""
    st = gait10dof18musc_marker_track(num_mesh_intervals, markers=markers, **kw)
    m = st.problem.model
    m.add_offset_frame("imu_r", "calcn_r", (0.1, 0.03, 0.0), (0.1, -0.2, 1.3))
    m.add_offset_frame("imu_l", "calcn_l", (0.1, 0.03, 0.0), (-0.1, 0.2, 1.3))
    data = _load("walk_gait1018_state_reference.json")
    states = DataTable("states_reference", np.asarray(data["time"]),
                       {k: np.asarray(v, float) for k, v in data["columns"].items()})
    goals = [MocoOrientationTrackingGoal("orientation_tracking", 1.0, states_reference=states,
                                         frame_paths=list(frames))]
    if translation:
        goals.append(MocoTranslationTrackingGoal("translation_tracking", 1.0, states_reference=states,
                                                 frame_paths=["/bodyset/pelvis"]))
    for g in goals:
        m.add_table(g.reference_table(m))
    st.problem.goals[1:1] = goals   # after the marker goal, before the effort goal
    return st


def gait10dof18musc_frame_track_few(num_mesh_intervals: int = 3, **kw) -> MocoStudy:
    """N = 3: orientation tracking of the pelvis, both femurs and both tibias,
    translation tracking of the pelvis, and a marker goal with two markers
    (pelvis, tibia_l off the body origin) -- all three item types in one
    launch."""
    return gait10dof18musc_frame_track(num_mesh_intervals, markers=(GAIT_MARKERS_FEW[0], GAIT_MARKERS_FEW[2]),
                                       frames=GAIT_ORIENTATION_FRAMES_FEW, translation=True, **kw)


def append_value_derivatives_as_speeds(states: DataTable, degree: int = 5) -> DataTable:
    """TableProcessor's appendCoordinateValueDerivativesAsSpeeds (what
    MocoTrack's track_reference_position_derivatives does): for every
    <coordinate>/value column without a <coordinate>/speed column, the speed
    is the derivative at the rows of the column's interpolating spline."""
    from .splines import gcv_interpolating_ppoly
    t = np.asarray(states.times, float)
    cols = dict(states.columns)
    for k, v in states.columns.items():
        sp = k[:-len("value")] + "speed"
        if not k.endswith("/value") or sp in cols:
            continue
        br, cf = gcv_interpolating_ppoly(t, np.asarray(v, float), degree)
        dt = br[-1] - br[-2]
        last = sum(n * cf[-1, 0, n] * dt ** (n - 1) for n in range(1, degree + 1))
        cols[sp] = np.append(cf[:, 0, 1], last)
    return DataTable(states.name, t, cols)


def gait10dof18musc_imu_track(num_mesh_intervals: int = 200, frames=GAIT_ORIENTATION_FRAMES,
                              **kw) -> MocoStudy:
    """gait10dof18musc_frame_track plus a MocoAngularVelocityTrackingGoal
    "angular_velocity_tracking" (weight 1, frame weights 1) on the same
    ``frames`` -- an inertial sensor's orientation and gyroscope rate per
    segment, one kinematics pass for both; the reference is computed from the
    bundled walking data's coordinate values and their derivatives as speeds
    (append_value_derivatives_as_speeds: the data has values only)."""
    st = gait10dof18musc_frame_track(num_mesh_intervals, frames=frames, **kw)
    m = st.problem.model
    data = _load("walk_gait1018_state_reference.json")
    states = DataTable("states_reference", np.asarray(data["time"]),
                       {k: np.asarray(v, float) for k, v in data["columns"].items()})
    g = MocoAngularVelocityTrackingGoal("angular_velocity_tracking", 1.0,
                                        states_reference=append_value_derivatives_as_speeds(states),
                                        frame_paths=list(frames))
    m.add_table(g.reference_table(m))
    st.problem.goals.insert(len(st.problem.goals) - 1, g)   # before the effort goal
    return st


def gait10dof18musc_imu_track_few(num_mesh_intervals: int = 3, **kw) -> MocoStudy:
    """N = 3: gait10dof18musc_frame_track_few plus angular-velocity tracking
    of the pelvis, both femurs and both tibias."""
    return gait10dof18musc_imu_track(num_mesh_intervals, markers=(GAIT_MARKERS_FEW[0], GAIT_MARKERS_FEW[2]),
                                     frames=GAIT_ORIENTATION_FRAMES_FEW, translation=True, **kw)


def spline_knee_model(slider_foot: bool = False) -> Model:
    """A thigh on a pin joint and a shank on a custom joint with one
    coordinate, knee, that drives -- in this axis order -- a rotation about z
    through a SimmSpline (seven knots, slope from 0.4 to 1.6), a rotation about
    x through a linear function (0.3 knee) and a translation along y through a
    SimmSpline: the coupled knee of a gait model, small.  CoordinateActuators
    on both coordinates, an offset frame "imu" on the shank.  ``slider_foot``:
    also a foot on a slider joint under the shank, whose coordinate turns
    nothing."""
    m = Model("spline_knee")
    m.add_body(Body("thigh", 2.0, (0, -0.2, 0), (0.1, 0.02, 0.1, 0, 0, 0)))
    m.add_body(Body("shank", 1.5, (0, -0.2, 0), (0.08, 0.01, 0.08, 0, 0, 0)))
    hip = Coordinate("hip", (-1.5, 1.5))
    knee = Coordinate("knee", (-2.0, 0.2))
    m.add_joint(Joint.pin("hip", "ground", "thigh", hip, loc_in_parent=(0, 1, 0)))
    kx = (-2.0, -1.6, -1.2, -0.8, -0.4, 0.0, 0.2)
    m.add_joint(Joint("knee", "thigh", "shank", [knee], [
        Axis(abi.MH_AXIS_ROTATION, (0, 0, 1),
             Function.simm_spline("knee", kx, (-2.32, -2.08, -1.72, -1.24, -0.66, 0.0, 0.32))),
        Axis(abi.MH_AXIS_ROTATION, (1, 0, 0), Function.linear("knee", 0.3)),
        Axis(abi.MH_AXIS_TRANSLATION, (0, 1, 0),
             Function.simm_spline("knee", kx, (-0.422, -0.4082, -0.399, -0.3976, -0.3966, -0.3952, -0.3946))),
    ], loc_in_parent=(0, -0.05, 0)))
    m.add_coordinate_actuator(CoordinateActuator("tau_hip", "hip", 10.0, path="/tau_hip"))
    m.add_coordinate_actuator(CoordinateActuator("tau_knee", "knee", 10.0, path="/tau_knee"))
    m.add_offset_frame("imu", "shank", (0.03, -0.15, 0.02), (0.2, 0.5, -0.4))
    if slider_foot:
        m.add_body(Body("foot", 0.5, (0.05, 0, 0), (0.01, 0.01, 0.01, 0, 0, 0)))
        slide = Coordinate("slide", (-0.1, 0.1), motion_type="translational")
        m.add_joint(Joint.slider("ankle", "shank", "foot", slide, loc_in_parent=(0, -0.4, 0)))
        m.add_coordinate_actuator(CoordinateActuator("tau_slide", "slide", 10.0, path="/tau_slide"))
    return m


def spline_knee_motion(times):
    """A smooth motion of (hip, knee) within their ranges, and its rates."""
    t = np.asarray(times, float)
    return ({"hip": 0.5 * np.sin(3.0 * t), "knee": -0.9 + 0.8 * np.cos(2.0 * t + 0.4)},
            {"hip": 1.5 * np.cos(3.0 * t), "knee": -1.6 * np.sin(2.0 * t + 0.4)})


def spline_knee(num_mesh_intervals: int = 2, scheme: str = "hermite-simpson", fd_scheme: str = "central",
                slider_foot: bool = False) -> MocoStudy:
    """spline_knee_model over [0, 0.6]: a MocoAngularVelocityTrackingGoal of
    the thigh, of the shank's "imu" frame (weight 2) and, with ``slider_foot``,
    of the foot, the reference computed along spline_knee_motion at 31 rows,
    plus a control-effort goal (0.001).  No generated back end: the device
    interpreter runs it."""
    m = spline_knee_model(slider_foot)
    imu = "/bodyset/shank/imu"
    paths = ["/bodyset/thigh", imu] + (["/bodyset/foot"] if slider_foot else [])
    times = np.linspace(0.0, 0.6, 31)
    q, u = spline_knee_motion(times)
    om = [[m.frame_angular_velocity_in_ground(f, {n: v[r] for n, v in q.items()}, {n: v[r] for n, v in u.items()})
           for f in paths] for r in range(len(times))]
    g = MocoAngularVelocityTrackingGoal("angular_velocity_tracking", 1.0,
                                        reference=FrameReference(times, paths, np.array(om)),
                                        frame_weights={imu: 2.0})
    m.add_table(g.reference_table(m))
    p = MocoProblem(m)
    p.set_time_bounds(0, 0.6)
    p.set_state_info("/jointset/hip/hip/value", (-1.5, 1.5))
    p.set_state_info("/jointset/hip/hip/speed", (-10, 10))
    p.set_state_info("/jointset/knee/knee/value", (-2.0, 0.2))
    p.set_state_info("/jointset/knee/knee/speed", (-10, 10))
    if slider_foot:
        p.set_state_info("/jointset/ankle/slide/value", (-0.1, 0.1))
        p.set_state_info("/jointset/ankle/slide/speed", (-1, 1))
    p.add_goal(g)
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme)
    return MocoStudy(p, s)


def scale_subject(m: Model, length: float = 1.03, mass: float = 1.05) -> Model:
    """A scaled subject (what OpenSim's ScaleTool produces from a generic
    model, uniformly): every length -- joint frame locations, centers of
    mass, path-point locations, CustomJoint translation splines and
    MovingPathPoint functions, optimal fiber and tendon slack lengths --
    times ``length``,
    masses times ``mass``, inertias times mass * length^2.  The model
    STRUCTURE is unchanged, so a generated back end of the generic model
    serves it (codegen.py "Structure-only specialization")."""
    L, W = float(length), float(mass)
    for b in m.bodies.values():
        b.mass *= W
        b.com = tuple(L * c for c in b.com)
        b.inertia = tuple(W * L * L * i for i in b.inertia)
    for j in m.joints:
        j.loc_in_parent = tuple(L * c for c in j.loc_in_parent)
        j.loc_in_child = tuple(L * c for c in j.loc_in_child)
        for ax in j.axes:
            # translations that are functions of a rotation (the knee's
            # SimmSplines, MultiplierFunction); a translational coordinate's
            # own linear function is a length already
            if (ax.type == abi.MH_AXIS_TRANSLATION and ax.func is not None
                    and ax.func.kind != abi.MH_FN_LINEAR):
                ax.func = ax.func.scaled(L)
    for mu in m.muscles:
        mu.optimal_fiber_length *= L
        mu.tendon_slack_length *= L
        for pt in mu.points:
            pt.loc = tuple(L * c for c in pt.loc)
            pt.fx, pt.fy, pt.fz = (f.scaled(L) if f is not None else None for f in (pt.fx, pt.fy, pt.fz))
    return m


def gait10dof18musc_track(num_mesh_intervals: int = 65, muscles: bool = False) -> MocoStudy:
    """The reference's MocoTrack golden-solution problem (testMocoTrack.cpp:
    46-68): gait10dof18musc | ModOpRemoveMuscles | ModOpAddReserves(100) |
    ModOpAddExternalLoads; states reference walk_gait1018_state_reference.mot
    | TabOpLowPassFilter(6) tracked with weight 1 (GCVSpline of degree 5),
    control effort 0.001, time [0.01, 1.3], mesh_interval 0.02 (N = 65),
    explicit dynamics, forward differences, convergence and constraint
    tolerances 1e-2, bounds guess (MocoTrack.cpp:54-132).  Its converged
    solution is std_testMocoTrackGait10dof18musc_solution.sto.

    muscles=True: BASELINE configs[2], the same MocoTrack with the 18
    muscles replaced by DeGrooteFregly2016Muscle (rigid tendons,
    ModOpReplaceMusclesWithDeGrooteFregly2016) instead of removed -- the
    muscle-driven workload the headline throughput is measured on, solved
    with MocoTrack's settings."""
    from .splines import filter_lowpass_table
    m = gait10dof18musc_model(muscles=muscles)
    ref = _load("walk_gait1018_state_reference.json")
    tp, cols = filter_lowpass_table(ref["time"], {k: np.asarray(v) for k, v in ref["columns"].items()}, 6.0)
    m.add_table(DataTable("state_reference", tp, cols, degree=5))
    p = MocoProblem(m)
    p.add_goal(MocoStateTrackingGoal("state_tracking", 1.0, DataTable("state_reference", tp, cols, degree=5)))
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    p.set_time_bounds(0.01, 1.3)
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, optim_finite_difference_scheme="forward",
                      optim_convergence_tolerance=1e-2, optim_constraint_tolerance=1e-2)
    return MocoStudy(p, s)


def gait10dof18musc_inverse(num_mesh_intervals: int = 25, fd_scheme: str = "forward",
                            sparsity: str = "random", subject=None, output_paths=()) -> MocoStudy:
    """MocoInverse on gait10dof18musc (configs[4], one solve of the batch):
    kinematics prescribed by a PositionMotion of the coordinate trajectories
    (MocoInverse.cpp:46-66; GCVSpline degree 5, PositionMotion.cpp:121-155),
    DeGrooteFregly2016 muscles with compliant tendons in implicit mode
    (testMocoInverse.cpp:120-130), reserves, ExternalLoads, control effort
    goal with reserves weight 1 (MocoInverse.cpp:89-90), the initial-
    activation endpoint constraint (MocoInverse.cpp:93), implicit dynamics,
    no control-midpoint interpolation, forward differences and "random"
    sparsity detection (MocoInverse.cpp:104-114).  The kinematics are the
    bundled walking coordinate trajectories, clipped by 1e-3 at both ends
    (clip_time_range, MocoInverse.cpp:82-86).  ``subject`` = (length,
    mass) scales the model (scale_subject: one subject of a configs[4]
    sweep; the same kinematics).  ``output_paths``: MocoInverse's property
    (MocoInverse.cpp:133-139): the solution of solve() carries
    analyze(solution, output_paths) as ``outputs``."""
    m = gait10dof18musc_model(tendon_compliance=True, tendon_dynamics="implicit")
    if subject is not None:
        m = scale_subject(m, *subject)
    ref = _load("walk_gait1018_state_reference.json")
    t = np.asarray(ref["time"])
    kin = DataTable("kinematics", t, {k: np.asarray(v) for k, v in ref["columns"].items()
                                      if k.endswith("/value")}, degree=5)
    p = MocoProblem(m)
    p.set_position_motion(kin)
    p.set_time_bounds(float(t[0]) + 1e-3, float(t[-1]) - 1e-3)
    p.add_goal(MocoControlGoal("excitation_effort", 1.0))
    # prevent "free" activation at the beginning of the motion (MocoInverse.cpp:93)
    p.add_goal(MocoInitialActivationGoal("initial_activation"))
    # minimize_implicit_auxiliary_derivatives, weight 0.01 (MocoInverse.cpp:106-107)
    p.add_goal(ImplicitAuxiliaryDerivativesTerm(weight=0.01))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals,
                      optim_finite_difference_scheme=fd_scheme, multibody_dynamics_mode="implicit",
                      interpolate_control_midpoints=False,   # MocoInverse.cpp:105
                      optim_sparsity_detection=sparsity,
                      # MocoInverse convergence / constraint tolerance
                      # defaults (MocoInverse.cpp:38-39, 108-109)
                      optim_convergence_tolerance=1e-3, optim_constraint_tolerance=1e-3)
    st = MocoStudy(p, s)
    st.output_paths = list(output_paths)
    return st


def wrapped_pendulum(num_mesh_intervals: int = 20, scheme: str = "hermite-simpson",
                     dynamics: str = "explicit", tendon_compliance: bool = False,
                     quadrant: str = "all") -> MocoStudy:
    # (compliant tendon: the angle range over which the path wraps, with
    # tendon slack and fiber lengths that keep the muscle near its optimal
    # fiber length there, so the explicit tendon dynamics stay regular)
    """A one-link pendulum (ModelFactory::createNLinkPendulum(1)) driven by a
    DeGrooteFregly2016 muscle whose path wraps over a WrapCylinder about the
    pin axis (the GeometryPath / WrapCylinder geometry of SURVEY §8 A9 on a
    model small enough for every kernel variant).  Not a BASELINE config."""
    from .model import DeGrooteFregly2016Muscle, PathPoint, WrapCylinder
    m = n_link_pendulum(1)
    m.add_wrap(WrapCylinder("pin_cyl", "ground", 0.1, 0.2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), quadrant))
    mu = DeGrooteFregly2016Muscle("flexor", [PathPoint("ground", (-0.3, 0.15, 0.05), name="origin"),
                                             PathPoint("b0", (-0.7, 0.12, -0.04), name="insertion")],
                                  max_isometric_force=200.0,
                                  optimal_fiber_length=0.22 if tendon_compliance else 0.2,
                                  tendon_slack_length=0.45 if tendon_compliance else 0.25,
                                  pennation_angle_at_optimal=0.1,
                                  path_wraps=[("pin_cyl", -1, -1)])
    mu.ignore_tendon_compliance = not tendon_compliance
    m.actuators = [a for a in m.actuators]
    m.add_muscle(mu)
    p = MocoProblem(m)
    p.set_time_bounds(0.0, 1.0)
    p.set_state_info("/jointset/j0/q0/value", (-1.0, -0.4) if tendon_compliance else (-1.5, 1.5),
                     -0.7 if tendon_compliance else 0.5)
    p.set_state_info("/jointset/j0/q0/speed", (-3, 3), 0)
    p.set_control_info("/tau0", (-50, 50))
    p.add_goal(MocoControlGoal())
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def _walk_armless_grf(m: Model):
    """ModOpAddExternalLoads(subject_walk_armless_external_loads.xml / grf_walk.xml):
    ground-expressed force, point and torque on calcn_r / calcn_l."""
    grf = _load("subject_walk_armless_grf.json")
    cols = {k: np.asarray(v) for k, v in grf["columns"].items()}
    m.add_table(DataTable("grf", np.asarray(grf["time"]), cols, degree=3))
    for ef in grf["external_forces"]:
        if ef["force_expressed_in_body"] != "ground" or ef["point_expressed_in_body"] != "ground":
            raise NotImplementedError("ExternalForce must be expressed in ground")
        m.add_external_force(ExternalForce(ef["name"], ef["body"], "grf", ef["force_identifier"],
                                           ef["point_identifier"], ef["torque_identifier"]))


def _walk_armless_kinematics(m: Model, lowpass: float = 6.0) -> DataTable:
    """TableProcessor("subject_walk_armless_coordinates.mot") |
    TabOpLowPassFilter(6), in radians, columns renamed to the model's
    coordinate value paths (extra columns dropped: kinematics_allow_extra_columns)."""
    from .splines import filter_lowpass_table
    kin = _load("subject_walk_armless_coordinates.json")
    byname = {c.name: c for c in m.coordinates()}
    cols = {byname[k].path + "/value": np.asarray(v) for k, v in kin["columns"].items() if k in byname}
    tp, fcols = filter_lowpass_table(kin["time"], cols, lowpass)
    return DataTable("kinematics", tp, fcols, degree=5)


def _replaced(m: Model, keep_path_wraps: bool = False) -> Model:
    """ModOpReplaceMusclesWithDeGrooteFregly2016 on a model stored with its
    Millard muscles' PathWrapSets: replaceMuscles copies the path points only
    (DeGrooteFregly2016Muscle.cpp:1007-1020), so the wraps go."""
    if not keep_path_wraps:
        for mu in m.muscles:
            mu.path_wraps = []
    return m


def rajagopal18_model(keep_path_wraps: bool = False) -> Model:
    """testMocoInverse.cpp:121-128: subject_walk_armless_18musc.osim |
    ModOpReplaceJointsWithWelds(subtalar, mtp) | ModOpReplaceMusclesWith
    DeGrooteFregly2016 | ModOpIgnorePassiveFiberForcesDGF |
    ModOpTendonComplianceDynamicsModeDGF("implicit") | ModOpAddExternalLoads.
    18 muscles over 16 PathWraps on WrapCylinders, 2 patellofemoral
    CoordinateCouplerConstraints, the model's own reserve actuators."""
    m = _replaced(model_from_dict(_load("rajagopal18.json")), keep_path_wraps)
    m.replace_joints_with_welds(["subtalar_r", "subtalar_l", "mtp_r", "mtp_l"])
    for mu in m.muscles:
        mu.ignore_passive_fiber_force = True
        mu.tendon_compliance_dynamics_mode = "implicit"
    _walk_armless_grf(m)
    return m


def rajagopal18_inverse(num_mesh_intervals: int = 11, fd_scheme: str = "forward",
                        sparsity: str = "random", keep_path_wraps: bool = False) -> MocoStudy:
    """MocoInverse Rajagopal2016, 18 muscles (testMocoInverse.cpp:118-147):
    time [0.45, 1.0], mesh_interval 0.05 (N = 11), kinematics low-pass
    filtered at 6 Hz and prescribed by a PositionMotion, the MocoInverse
    goals and solver settings (MocoInverse.cpp:46-120; see
    gait10dof18musc_inverse).  The coupler multipliers stay NLP variables
    (constraint forces in the residual), without kinematic rows.  Its
    converged solution is std_testMocoInverse_subject_18musc_solution.sto.
    keep_path_wraps=True keeps the Millard muscles' PathWraps (16 on
    WrapCylinders), which the reference's replaceMuscles drops."""
    m = rajagopal18_model(keep_path_wraps)
    kin = _walk_armless_kinematics(m)
    p = MocoProblem(m)
    p.set_position_motion(kin)
    p.set_time_bounds(0.45, 1.0)
    p.add_goal(MocoControlGoal("excitation_effort", 1.0))
    p.add_goal(MocoInitialActivationGoal("initial_activation"))
    p.add_goal(ImplicitAuxiliaryDerivativesTerm(weight=0.01))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals,
                      optim_finite_difference_scheme=fd_scheme, multibody_dynamics_mode="implicit",
                      interpolate_control_midpoints=False, optim_sparsity_detection=sparsity,
                      optim_convergence_tolerance=1e-3, optim_constraint_tolerance=1e-3)
    return MocoStudy(p, s)


def rajagopal80_model(keep_path_wraps: bool = False) -> Model:
    """example3DWalking muscleDrivenStateTracking (exampleMocoTrack.cpp):
    subject_walk_armless.osim | ModOpAddExternalLoads(grf_walk.xml) |
    ModOpIgnoreTendonCompliance | ModOpReplaceMusclesWithDeGrooteFregly2016 |
    ModOpIgnorePassiveFiberForcesDGF | ModOpScaleActiveFiberForceCurveWidthDGF(1.5):
    80 DGF muscles (rigid tendons; their 46 PathWraps dropped by
    replaceMuscles unless keep_path_wraps), 18 coordinates, 2 patellofemoral
    couplers, the model's 6 pelvis actuators."""
    m = _replaced(model_from_dict(_load("rajagopal80.json")), keep_path_wraps)
    for mu in m.muscles:
        mu.ignore_tendon_compliance = True
        mu.ignore_passive_fiber_force = True
        mu.active_force_width_scale = 1.5
    _walk_armless_grf(m)
    return m


def rajagopal80(num_mesh_intervals: int = 400, fd_scheme: str = "forward",
                scheme: str = "hermite-simpson", keep_path_wraps: bool = False) -> MocoStudy:
    """BASELINE configs[3]: the Rajagopal 80-muscle gait NLP at N = 400.  The
    reference's 80-muscle problem (example3DWalking exampleMocoTrack.cpp
    muscleDrivenStateTracking: states tracking weight 10, control effort,
    time [0.81, 1.65], explicit dynamics with the patellofemoral couplers
    and their derivatives enforced, forward FD) on the filtered coordinate
    trajectories; BASELINE names a predictive problem, whose contact models
    are outside this path, so the goals here are the tracking example's
    (the NLP's layout, DAE and Jacobian are the same).  Block-dense callback
    sparsity (detection with kinematic constraints is rejected: SURVEY §8
    F2 note in DESIGN.md).  keep_path_wraps=True: with the 46 PathWraps."""
    m = rajagopal80_model(keep_path_wraps)
    kin = _walk_armless_kinematics(m)
    m.add_table(DataTable("state_reference", kin.times, kin.columns, degree=5))
    p = MocoProblem(m)
    p.add_goal(MocoStateTrackingGoal("state_tracking", 10.0, DataTable(
        "state_reference", kin.times, kin.columns, degree=5)))
    p.add_goal(MocoControlGoal("control_effort", 1.0))
    p.set_time_bounds(0.81, 1.65)
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme)
    return MocoStudy(p, s)


CONFIGS = {
    "sliding_mass": sliding_mass,
    "double_pendulum": double_pendulum,
    "double_pendulum_swingup": double_pendulum_swingup,
    "double_pendulum_coupled": double_pendulum_coupled,
    "gait10dof18musc": gait10dof18musc,
    "gait10dof18musc_inverse": gait10dof18musc_inverse,
    "gait10dof18musc_track": gait10dof18musc_track,
    "double_pendulum_marker_tracking": double_pendulum_marker_tracking,
    "gait10dof18musc_marker_track": gait10dof18musc_marker_track,
    "gait10dof18musc_marker_track_few": gait10dof18musc_marker_track_few,
    "double_pendulum_effort": double_pendulum_effort,
    "double_pendulum_frame_tracking": double_pendulum_frame_tracking,
    "gimbal_frame_tracking": gimbal_frame_tracking,
    "gait10dof18musc_frame_track": gait10dof18musc_frame_track,
    "gait10dof18musc_frame_track_few": gait10dof18musc_frame_track_few,
    "gait10dof18musc_imu_track": gait10dof18musc_imu_track,
    "gait10dof18musc_imu_track_few": gait10dof18musc_imu_track_few,
    "spline_knee": spline_knee,
    "wrapped_pendulum": wrapped_pendulum,
    "rajagopal18_inverse": rajagopal18_inverse,
    "rajagopal80": rajagopal80,
}


# ---- MocoJointReactionGoal ---------------------------------------------------
def double_pendulum_joint_reaction(num_mesh_intervals: int = 2, scheme: str = "hermite-simpson",
                                   fd_scheme: str = "central", dynamics: str = "explicit",
                                   reaction: bool = True) -> MocoStudy:
    """The double pendulum (control-effort goal, 0.001) over [0, 1] with three
    MocoJointReactionGoals on its second pin, j1, after it: "reaction_child"
    (weight 0.5: the loads on the child frame, all six measures, force-y
    weighted 2), "reaction_parent" (weight 0.25: the loads on the parent frame
    expressed in the rotated offset frame "probe" of b0) and "reaction_subset"
    (the parent loads in ground, moment-z and force-x only, force-x weighted
    3).  ``reaction`` = False: the same study without them."""
    m = n_link_pendulum(2)
    m.add_offset_frame("probe", "b0", (-0.3, 0.1, 0.05), (0.3, -0.6, 0.9))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, 1.0)
    for j, q in (("j0", "q0"), ("j1", "q1")):
        p.set_state_info(f"/jointset/{j}/{q}/value", (-10, 10))
        p.set_state_info(f"/jointset/{j}/{q}/speed", (-50, 50))
    p.set_control_info("/tau0", (-100, 100))
    p.set_control_info("/tau1", (-100, 100))
    p.add_goal(MocoControlGoal("control_effort", 0.001))
    if reaction:
        p.add_goal(MocoJointReactionGoal("reaction_child", 0.5, joint_path="/jointset/j1", loads_frame="child",
                                         reaction_weights={"force-y": 2.0}))
        p.add_goal(MocoJointReactionGoal("reaction_parent", 0.25, joint_path="j1",
                                         expressed_in_frame_path="/bodyset/b0/probe"))
        p.add_goal(MocoJointReactionGoal("reaction_subset", 1.0, joint_path="j1",
                                         expressed_in_frame_path="/ground",
                                         reaction_measures=["force-x", "moment-z"],
                                         reaction_weights={"force-x": 3.0}))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme, multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def spline_knee_weld(num_mesh_intervals: int = 2, fd_scheme: str = "central", dynamics: str = "explicit",
                     reaction: bool = True) -> MocoStudy:
    """spline_knee's study (spline and translation axes) with a "brace" of
    mass 0.4 welded to the shank at (0.02, -0.25, 0.01), rotated by (0.1,
    -0.2, 0.3), and two MocoJointReactionGoals: "knee_reaction" (the knee's
    loads on its child, the shank, in the shank's "imu" frame) and
    "weld_reaction" (the weld's loads on its parent frame).  ``reaction`` =
    False: the same study without them."""
    st = spline_knee(num_mesh_intervals, fd_scheme=fd_scheme)
    m = st.problem.model
    m.add_body(Body("brace", 0.4, (0.01, -0.03, 0.02), (0.004, 0.003, 0.005, 0, 0, 0)))
    m.add_joint(Joint("brace_weld", "shank", "brace", [], [], loc_in_parent=(0.02, -0.25, 0.01),
                      orient_in_parent=(0.1, -0.2, 0.3), loc_in_child=(0.0, 0.05, 0.0)))
    if reaction:
        st.problem.add_goal(MocoJointReactionGoal("knee_reaction", 0.5, joint_path="knee", loads_frame="child",
                                                  expressed_in_frame_path="/bodyset/shank/imu"))
        st.problem.add_goal(MocoJointReactionGoal("weld_reaction", 2.0, joint_path="brace_weld"))
    st.solver.multibody_dynamics_mode = dynamics
    return st


def cart_welded_payload(num_mesh_intervals: int = 5) -> MocoStudy:
    """A cart A (mass 1) on a slider along x with a CoordinateActuator and a
    payload B (mass 1) welded to it, gravity (10, 0, 0) along the slider, time
    [0, 1], from rest at 0, control in [-20, 20]: minimize force-x of the weld.
    The weld carries nothing exactly in free fall: control 0, final position
    5, final speed 10 (the slider stand-in for testMocoGoals.cpp:364-411, whose
    PointActuator on a coordinate-free model is not available here)."""
    m = Model("cart_welded_payload", gravity=(10.0, 0.0, 0.0))
    m.add_body(Body("A", 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
    m.add_body(Body("B", 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
    x = Coordinate("x", (-math.inf, math.inf), "translational")
    m.add_joint(Joint.slider("slider", "ground", "A", x))
    m.add_joint(Joint("weld", "A", "B", [], [], loc_in_parent=(0.0, 0.5, 0.0)))
    m.add_coordinate_actuator(CoordinateActuator("push", "x", 1.0, path="/forceset/push"))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, 1.0)
    p.set_state_info("/jointset/slider/x/value", (-20, 20), 0)
    p.set_state_info("/jointset/slider/x/speed", (-50, 50), 0)
    p.set_control_info("/forceset/push", (-20, 20))
    p.add_goal(MocoJointReactionGoal("weld_force", 1.0, joint_path="weld", reaction_measures=["force-x"]))
    return MocoStudy(p, MocoHipSolver(num_mesh_intervals=num_mesh_intervals))


def inverted_pendulum(num_mesh_intervals: int = 20, goal: str = "effort") -> MocoStudy:
    """exampleMinimizeJointReaction.m:44-106: a body (mass 1, inertia 1) on a
    pin at the ground origin, joint frame at (-1, 0, 0) of the body, a
    CoordinateActuator of optimal force 1, time [0, 1], the angle from 0 to pi
    at rest, control in [-100, 100], convergence tolerance 1e-3.  goal:
    "effort" (MocoControlGoal) or "reaction" (MocoJointReactionGoal on the pin,
    its defaults)."""
    m = Model("inverted_pendulum")
    m.add_body(Body("body", 1.0, (0, 0, 0), (1, 1, 1, 0, 0, 0)))
    angle = Coordinate("angle", (-math.inf, math.inf))
    m.add_joint(Joint.pin("pin", "ground", "body", angle, loc_in_child=(-1, 0, 0)))
    m.add_coordinate_actuator(CoordinateActuator("actuator", "angle", 1.0, path="/forceset/actuator"))
    m.add_offset_frame("body_center", "body", (-0.5, 0.0, 0.0))
    p = MocoProblem(m)
    p.set_time_bounds(0.0, 1.0)
    p.set_state_info("/jointset/pin/angle/value", (-10, 10), 0, math.pi)
    p.set_state_info("/jointset/pin/angle/speed", (-50, 50), 0, 0)
    p.set_control_info("/forceset/actuator", (-100, 100))
    if goal == "effort":
        p.add_goal(MocoControlGoal("effort"))
    elif goal == "reaction":
        p.add_goal(MocoJointReactionGoal("reaction", joint_path="pin"))
    else:
        raise ValueError(goal)
    return MocoStudy(p, MocoHipSolver(num_mesh_intervals=num_mesh_intervals, optim_convergence_tolerance=1e-3))


def gait10dof18musc_knee_reaction(num_mesh_intervals: int = 200, joint: str = "knee_r", **kw) -> MocoStudy:
    """gait10dof18musc's study with a MocoJointReactionGoal "knee_reaction"
    (weight 0.1) after its goals: the loads of ``joint`` on its child frame,
    all six measures."""
    st = gait10dof18musc(num_mesh_intervals, **kw)
    st.problem.add_goal(MocoJointReactionGoal("knee_reaction", 0.1, joint_path=joint, loads_frame="child"))
    return st


# ---- MocoAccelerationTrackingGoal ----------------------------------------------
def accelerations_from_coordinates(m: Model, paths, times, coordinate_columns) -> FrameReference:
    """A reference for a MocoAccelerationTrackingGoal from coordinate data
    alone: the second time difference (numpy.gradient applied twice, second-
    order edges) of the frames' origin positions by forward kinematics at the
    rows.  Data to track, not a check of anything."""
    t = np.asarray(times, float)
    pos = np.array([[m.frame_pose_in_ground(f, {n: v[r] for n, v in coordinate_columns.items()})[0] for f in paths]
                    for r in range(len(t))])
    vel = np.gradient(pos, t, axis=0, edge_order=2)
    return FrameReference(t, list(paths), np.gradient(vel, t, axis=0, edge_order=2))


def double_pendulum_acceleration_tracking(reference: FrameReference = None, num_mesh_intervals: int = 20,
                                          scheme: str = "hermite-simpson", fd_scheme: str = "central",
                                          dynamics: str = "explicit") -> MocoStudy:
    """testMocoGoals.cpp:327-361: the effort problem with the effort goal's
    weight 0.001 and a MocoAccelerationTrackingGoal "tracking" on the frames
    /bodyset/b0 and /bodyset/b1.  ``reference``: the two frames' linear
    accelerations (the test: the effort solution's, HipNLP.
    frame_accelerations); None: those of double_pendulum_swing_states by
    accelerations_from_coordinates."""
    st = double_pendulum_effort(num_mesh_intervals, scheme, effort_weight=0.001)
    st.solver.optim_finite_difference_scheme = fd_scheme
    st.solver.multibody_dynamics_mode = dynamics
    m = st.problem.model
    paths = ["/bodyset/b0", "/bodyset/b1"]
    if reference is None:
        sw = double_pendulum_swing_states()
        reference = accelerations_from_coordinates(m, paths, sw.times, {
            "q0": sw.columns["/jointset/j0/q0/value"], "q1": sw.columns["/jointset/j1/q1/value"]})
    g = MocoAccelerationTrackingGoal("tracking", 1.0, reference=reference, frame_paths=paths)
    m.add_table(g.reference_table(m))
    st.problem.add_goal(g)
    return st


GAIT_ACCELERATION_FRAMES = ("/bodyset/pelvis", "/bodyset/tibia_r", "/bodyset/torso/imu_torso")


def gait10dof18musc_accel_track(num_mesh_intervals: int = 200, dynamics: str = "explicit",
                                frames=GAIT_ACCELERATION_FRAMES, **kw) -> MocoStudy:
    """gait10dof18musc's study (``dynamics``: explicit or implicit multibody
    dynamics) with a MocoAccelerationTrackingGoal "acceleration_tracking"
    (weight 0.01; the torso sensor weighted 2) before its effort goal: the
    accelerometer half of an inertial-sensor set on the pelvis, the right
    tibia and an offset frame "imu_torso" on the torso at (-0.05, 0.3, 0.02).
    The reference: accelerations_from_coordinates at the bundled walking
    data's rows."""
    st = gait10dof18musc(num_mesh_intervals, dynamics=dynamics, **kw)
    m = st.problem.model
    m.add_offset_frame("imu_torso", "torso", (-0.05, 0.3, 0.02), (0.2, -0.1, 0.4))
    data = _load("walk_gait1018_state_reference.json")
    bypath = {c.path + "/value": c.name for c in m.coordinates()}
    cols = {bypath[k]: np.asarray(v, float) for k, v in data["columns"].items() if k in bypath}
    imu = "/bodyset/torso/imu_torso"
    g = MocoAccelerationTrackingGoal("acceleration_tracking", 0.01,
                                     reference=accelerations_from_coordinates(m, frames, data["time"], cols),
                                     frame_weights={imu: 2.0} if imu in frames else {})
    m.add_table(g.reference_table(m))
    st.problem.goals.insert(len(st.problem.goals) - 1, g)   # before the effort goal
    return st


def gait10dof18musc_accel_track_few(num_mesh_intervals: int = 3, **kw) -> MocoStudy:
    """N = 3: gait10dof18musc_accel_track, for tests."""
    return gait10dof18musc_accel_track(num_mesh_intervals, **kw)


# ---- MocoOutputGoal over muscle outputs -------------------------------------
HANGING_MUSCLE_MASS = 0.5
HANGING_MUSCLE_GRAVITY = 9.81


def hanging_muscle(num_mesh_intervals: int = 5, tendon: str = "rigid", ignore_activation_dynamics: bool = False,
                   ignore_passive_fiber_force: bool = False, dynamics: str = "explicit",
                   scheme: str = "hermite-simpson", fd_scheme: str = "central", hold=None,
                   fiber_damping: float = 0.01) -> MocoStudy:
    """The hanging muscle of testMocoActuators.cpp (createHangingMuscleModel):
    a 0.5 kg mass on a SliderJoint along x, gravity 9.81 along +x, hanging from
    a DeGrooteFregly2016Muscle "actuator" that runs straight from the ground
    origin to the body origin, so that the muscle-tendon length is the
    coordinate "height" and its lengthening speed the coordinate's speed.
    ``tendon``: "rigid", or the compliant tendon's dynamics mode "explicit" /
    "implicit".  The goal is an effort goal; ``hold`` = a height: the position
    is bounded to that value and the speed to 0 over [0, 0.5] s, and the goal is
    a MocoOutputGoal on the tendon force divided by the mass (every feasible
    point then carries the weight: the integral is g times the duration)."""
    from .model import DeGrooteFregly2016Muscle, PathPoint
    m = Model("hanging_muscle", gravity=(HANGING_MUSCLE_GRAVITY, 0, 0))
    m.add_body(Body("body", HANGING_MUSCLE_MASS, (0, 0, 0), (0, 0, 0, 0, 0, 0)))
    height = Coordinate("height", (0.0, 0.3), "translational")
    m.add_joint(Joint.slider("joint", "ground", "body", height))
    mu = DeGrooteFregly2016Muscle("actuator", [PathPoint("ground", (0, 0, 0), name="origin"),
                                               PathPoint("body", (0, 0, 0), name="insertion")],
                                  max_isometric_force=30.0, optimal_fiber_length=0.10, tendon_slack_length=0.05,
                                  pennation_angle_at_optimal=0.1, max_contraction_velocity=10.0,
                                  fiber_damping=fiber_damping, tendon_strain_at_one_norm_force=0.10)
    mu.ignore_tendon_compliance = tendon == "rigid"
    mu.tendon_compliance_dynamics_mode = "implicit" if tendon == "implicit" else "explicit"
    mu.ignore_activation_dynamics = ignore_activation_dynamics
    mu.ignore_passive_fiber_force = ignore_passive_fiber_force
    m.add_muscle(mu)
    p = MocoProblem(m)
    if hold is None:
        p.set_time_bounds(0.0, (0.05, 1.0))
        p.set_state_info("/jointset/joint/height/value", (0.10, 0.20), 0.15, 0.14)
        p.set_state_info("/jointset/joint/height/speed", (-1.0, 1.0), 0.0, 0.0)
        p.add_goal(MocoControlGoal("effort", 1.0))
    else:
        p.set_time_bounds(0.0, 0.5)
        p.set_state_info("/jointset/joint/height/value", (float(hold), float(hold)))
        p.set_state_info("/jointset/joint/height/speed", (0.0, 0.0))
        p.add_goal(MocoOutputGoal("carried_weight", 1.0, output_path="/forceset/actuator|tendon_force",
                                  divide_by_mass=True))
    s = MocoHipSolver(num_mesh_intervals=num_mesh_intervals, transcription_scheme=scheme,
                      optim_finite_difference_scheme=fd_scheme, multibody_dynamics_mode=dynamics)
    return MocoStudy(p, s)


def gait10dof18musc_muscle_outputs(num_mesh_intervals: int = 200, output: str = "active_fiber_force",
                                   weight: float = 1e-4, **kw) -> MocoStudy:
    """gait10dof18musc's study with one MocoOutputGoal per muscle on ``output``
    (18 goals, before the effort goal): the profile's workload."""
    st = gait10dof18musc(num_mesh_intervals, **kw)
    for mu in st.problem.model.muscles:
        st.problem.goals.insert(len(st.problem.goals) - 1,
                                MocoOutputGoal(f"{output}_{mu.name}", weight, output_path=f"{mu.path}|{output}"))
    return st


# ---- MocoOutputGoal over a Bhargava2004Metabolics component -------------------
def hanging_muscle_metabolics(num_mesh_intervals: int = 5, output: str = "total_metabolic_rate",
                              divide_by_mass: bool = False, weight: float = 1.0, muscle_mass: float = float("nan"),
                              ratio_slow_twitch_fibers: float = 0.5, **kw) -> MocoStudy:
    """hanging_muscle with a Bhargava2004Metabolics component "metabolics" over
    its muscle and one MocoOutputGoal "met" on ``/metabolics|<output>`` as the
    only goal.  Keywords that are properties of the component
    (use_smoothing, smoothing_type, include_negative_mechanical_work, ...) go
    to it, the others to hanging_muscle."""
    from .model import Bhargava2004Metabolics
    own = {k: kw.pop(k) for k in list(kw) if k in Bhargava2004Metabolics.__dataclass_fields__}
    st = hanging_muscle(num_mesh_intervals, **kw)
    met = Bhargava2004Metabolics("metabolics", **own)
    met.add_muscle("actuator", "/forceset/actuator", ratio_slow_twitch_fibers=ratio_slow_twitch_fibers,
                   muscle_mass=muscle_mass)
    st.problem.model.add_component(met)
    st.problem.goals = [MocoOutputGoal("met", weight, output_path="/metabolics|" + output,
                                       divide_by_mass=divide_by_mass)]
    return st


def gait10dof18musc_metabolics(num_mesh_intervals: int = 200, smoothing: str = "tanh", weight: float = 0.1,
                               **kw) -> MocoStudy:
    """gait10dof18musc's study with a Bhargava2004Metabolics component
    "metabolics" over all 18 muscles (use_smoothing, ``smoothing`` = "tanh" or
    "huber") and a MocoOutputGoal "met" on its total metabolic rate divided by
    the model's mass, before the effort goal, as example2DWalkingMetabolics
    sets its metabolic cost up."""
    from .model import Bhargava2004Metabolics
    st = gait10dof18musc(num_mesh_intervals, **kw)
    met = Bhargava2004Metabolics("metabolics", use_smoothing=True, smoothing_type=smoothing)
    for mu in st.problem.model.muscles:
        met.add_muscle(mu.name, mu.path)
    st.problem.model.add_component(met)
    st.problem.goals.insert(len(st.problem.goals) - 1,
                            MocoOutputGoal("met", weight, output_path="/metabolics|total_metabolic_rate",
                                           divide_by_mass=True))
    return st
