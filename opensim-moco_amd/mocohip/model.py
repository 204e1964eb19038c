"""Host-side model compiler: OpenSim-like model objects -> mh_model tape.

This mirrors the parts of OpenSim's Model that the collocation hot path
reads (bodies/joints/coordinates, DeGrooteFregly2016 muscles with their
GeometryPath, CoordinateActuators, ExternalForces) and lowers them to the
plain C structs of include/mocohip.h.

Ordering rules restated from the reference:
  * generalized coordinates follow Simbody's mobilized-body order, which
    OpenSim's MultibodyGraphMaker grows one tree level at a time (joints in
    model order within a level) -- pinned by the column order of
    Moco/Tests/std_testMocoTrackGait10dof18musc_solution.sto:14;
  * auxiliary states per muscle: activation, then normalized tendon force
    (DeGrooteFregly2016Muscle.cpp:151-164); muscles in force-set order;
  * controls: actuators in component order (MocoUtilities.cpp:557-587).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .splines import gcv_interpolating_ppoly


# --------------------------------------------------------------------------
# Functions of one coordinate.
# --------------------------------------------------------------------------
@dataclass
class Function:
    kind: int
    coord: Optional[str] = None
    a: float = 0.0
    b: float = 0.0
    scale: float = 1.0
    x: Sequence[float] = ()
    y: Sequence[float] = ()

    @staticmethod
    def constant(v: float) -> "Function":
        return Function(abi.MH_FN_CONSTANT, None, a=float(v))

    @staticmethod
    def linear(coord: str, slope: float = 1.0, intercept: float = 0.0,
               scale: float = 1.0) -> "Function":
        return Function(abi.MH_FN_LINEAR, coord, a=float(slope),
                        b=float(intercept), scale=float(scale))

    @staticmethod
    def simm_spline(coord: str, x, y, scale: float = 1.0) -> "Function":
        return Function(abi.MH_FN_SIMMSPLINE, coord, x=list(map(float, x)),
                        y=list(map(float, y)), scale=float(scale))

    def scaled(self, s: float) -> "Function":
        """MultiplierFunction."""
        if self.kind == abi.MH_FN_CONSTANT:
            return Function.constant(self.a * s)
        f = Function(self.kind, self.coord, self.a, self.b, self.scale * s,
                     self.x, self.y)
        return f


# --------------------------------------------------------------------------
# Frames / rotations.
# --------------------------------------------------------------------------
def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], float)


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], float)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], float)


def _mm3(A, B):
    """3x3 product with each entry summed left to right (no BLAS): the same
    IEEE operations as the C++ builder (csrc/host/mh_builder.cpp mm3)."""
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)]
            for i in range(3)]


def body_fixed_xyz(angles) -> np.ndarray:
    """OpenSim frame orientation: Euler XYZ body-fixed angles,
    rot_x(a0) rot_y(a1) rot_z(a2)."""
    X, Y, Z = (r(float(a)).tolist() for r, a in zip((rot_x, rot_y, rot_z), angles))
    return np.array(_mm3(_mm3(X, Y), Z), float)


def unit3(d) -> List[float]:
    """d / |d| with |d| = sqrt((d0 d0 + d1 d1) + d2 d2) (as the C++ builder)."""
    d0, d1, d2 = (float(v) for v in d)
    n = math.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
    return [d0 / n, d1 / n, d2 / n]


@dataclass
class Body:
    name: str
    mass: float
    com: Sequence[float] = (0.0, 0.0, 0.0)
    inertia: Sequence[float] = (0, 0, 0, 0, 0, 0)   # xx yy zz xy xz yz


@dataclass
class Coordinate:
    name: str
    range: Sequence[float] = (-math.inf, math.inf)
    motion_type: str = "rotational"
    default_value: float = 0.0
    path: str = ""        # OpenSim absolute path, e.g. /jointset/j/q


@dataclass
class Axis:
    type: int            # abi.MH_AXIS_ROTATION / TRANSLATION
    dir: Sequence[float]
    func: Function


@dataclass
class Joint:
    name: str
    parent: str          # body name or "ground"
    child: str
    coordinates: List[Coordinate]
    axes: List[Axis]
    loc_in_parent: Sequence[float] = (0, 0, 0)
    orient_in_parent: Sequence[float] = (0, 0, 0)
    loc_in_child: Sequence[float] = (0, 0, 0)
    orient_in_child: Sequence[float] = (0, 0, 0)

    @staticmethod
    def pin(name, parent, child, coord: Coordinate, **frames) -> "Joint":
        """PinJoint: rotation about z of the joint frame."""
        return Joint(name, parent, child, [coord],
                     [Axis(abi.MH_AXIS_ROTATION, (0, 0, 1),
                           Function.linear(coord.name))], **frames)

    @staticmethod
    def slider(name, parent, child, coord: Coordinate, **frames) -> "Joint":
        """SliderJoint: translation along x of the joint frame."""
        return Joint(name, parent, child, [coord],
                     [Axis(abi.MH_AXIS_TRANSLATION, (1, 0, 0),
                           Function.linear(coord.name))], **frames)

    @staticmethod
    def planar(name, parent, child, rz: Coordinate, tx: Coordinate,
               ty: Coordinate, **frames) -> "Joint":
        """PlanarJoint: rotation about z, translation along x and y."""
        return Joint(name, parent, child, [rz, tx, ty], [
            Axis(abi.MH_AXIS_ROTATION, (0, 0, 1), Function.linear(rz.name)),
            Axis(abi.MH_AXIS_TRANSLATION, (1, 0, 0), Function.linear(tx.name)),
            Axis(abi.MH_AXIS_TRANSLATION, (0, 1, 0), Function.linear(ty.name)),
        ], **frames)

    @staticmethod
    def gimbal(name, parent, child, qx: Coordinate, qy: Coordinate, qz: Coordinate,
               **frames) -> "Joint":
        """GimbalJoint: rotations about x, y, z of the joint frame in
        body-fixed order."""
        return Joint(name, parent, child, [qx, qy, qz], [
            Axis(abi.MH_AXIS_ROTATION, (1, 0, 0), Function.linear(qx.name)),
            Axis(abi.MH_AXIS_ROTATION, (0, 1, 0), Function.linear(qy.name)),
            Axis(abi.MH_AXIS_ROTATION, (0, 0, 1), Function.linear(qz.name)),
        ], **frames)

    @staticmethod
    def weld(name, parent, child, **frames) -> "Joint":
        return Joint(name, parent, child, [], [], **frames)


@dataclass
class PathPoint:
    body: str
    loc: Sequence[float]
    kind: int = abi.MH_PP_FIXED
    coord: Optional[str] = None         # conditional
    range: Sequence[float] = (0.0, 0.0)
    fx: Optional[Function] = None       # moving
    fy: Optional[Function] = None
    fz: Optional[Function] = None
    name: str = ""


@dataclass
class DeGrooteFregly2016Muscle:
    """Properties and defaults of DeGrooteFregly2016Muscle
    (DeGrooteFregly2016Muscle.cpp:52-63)."""
    name: str
    points: List[PathPoint]
    max_isometric_force: float = 1000.0
    optimal_fiber_length: float = 0.1
    tendon_slack_length: float = 0.2
    pennation_angle_at_optimal: float = 0.0
    max_contraction_velocity: float = 10.0
    activation_time_constant: float = 0.015
    deactivation_time_constant: float = 0.060
    default_activation: float = 0.5
    default_normalized_tendon_force: float = 0.5
    active_force_width_scale: float = 1.0
    fiber_damping: float = 0.0
    passive_fiber_strain_at_one_norm_force: float = 0.6
    tendon_strain_at_one_norm_force: float = 0.049
    ignore_passive_fiber_force: bool = False
    ignore_activation_dynamics: bool = False
    ignore_tendon_compliance: bool = False
    tendon_compliance_dynamics_mode: str = "explicit"
    min_control: float = 0.0
    max_control: float = 1.0
    path: str = ""
    # GeometryPath PathWrapSet, in order: (wrap object name, range begin,
    # range end) with OpenSim's 1-based point range (< 1: first / last)
    path_wraps: List[tuple] = field(default_factory=list)


@dataclass
class WrapCylinder:
    """OpenSim WrapCylinder in a body's WrapObjectSet: axis = the z axis of
    its frame, which is rotated by the body-fixed X-Y-Z sequence
    ``xyz_body_rotation`` and translated by ``translation`` in the body;
    ``quadrant`` "all" / "+x" / "-x" / "+y" / "-y" (include/mocohip.h
    mh_wrap_object)."""
    name: str
    body: str
    radius: float
    length: float = 1.0
    xyz_body_rotation: Sequence[float] = (0.0, 0.0, 0.0)
    translation: Sequence[float] = (0.0, 0.0, 0.0)
    quadrant: str = "all"
    active: bool = True


def quadrant_axis_sign(quadrant: str):
    """WrapObject quadrant -> (wrap axis, wrap sign); "all" -> (0, 0)."""
    q = quadrant.strip().lower()
    if q in ("all", ""):
        return 0, 0
    sign = -1 if q.startswith("-") else 1
    ax = q.lstrip("+-")
    if ax not in ("x", "y", "z"):
        raise ValueError(f"bad wrap quadrant {quadrant!r}")
    if ax == "z":
        raise NotImplementedError("WrapCylinder quadrant along its axis")
    return "xy".index(ax), sign


@dataclass
class CoordinateActuator:
    name: str
    coordinate: str
    optimal_force: float = 1.0
    min_control: float = -math.inf
    max_control: float = math.inf
    path: str = ""


@dataclass
class SpringGeneralizedForce:
    """OpenSim SpringGeneralizedForce (opensim-core, third-party): the
    generalized force -stiffness (q - rest_length) - viscosity u on one
    coordinate (include/mocohip.h mh_spring; testMocoParameters.cpp:52-57);
    path /forceset/<name>."""
    name: str
    coordinate: str
    stiffness: float = 0.0
    rest_length: float = 0.0
    viscosity: float = 0.0
    path: str = ""


@dataclass
class Marker:
    """OpenSim::Marker: a point fixed on a body (``location`` in the body
    frame); path /markerset/<name>."""
    name: str
    body: str                # body name or "ground"
    location: Sequence[float] = (0.0, 0.0, 0.0)
    path: str = ""


@dataclass
class OffsetFrame:
    """OpenSim::PhysicalOffsetFrame on a body (or ground); path
    /bodyset/<body>/<name> (/ground/<name>): the translation, and the
    orientation as body-fixed XYZ angles (PhysicalOffsetFrame's
    ``orientation``; zeros unless given, and then not serialised)."""
    name: str
    body: str                # body name or "ground"
    translation: Sequence[float] = (0.0, 0.0, 0.0)
    path: str = ""
    orientation: Sequence[float] = (0.0, 0.0, 0.0)

    def oriented(self) -> bool:
        return any(float(v) != 0.0 for v in self.orientation)


@dataclass
class DataTable:
    """Time series; splined with the GCVSpline restatement (splines.py)."""
    name: str
    times: np.ndarray
    columns: Dict[str, np.ndarray]
    degree: int = 3
    # explicit piecewise polynomial (breaks[nseg+1], coefs[nseg, ncol,
    # degree+1]) instead of splining the samples (path-constraint bounds)
    ppoly: Optional[tuple] = None


@dataclass
class ExternalForce:
    name: str
    body: str
    table: str
    force_identifier: Optional[str] = None     # e.g. "ground_force_v"
    point_identifier: Optional[str] = None
    torque_identifier: Optional[str] = None


@dataclass
class Station:
    """OpenSim Station: a point fixed in a body (``location`` in the body's
    frame).  Path ``/<name>`` unless given."""
    name: str
    body: str
    location: Sequence[float] = (0.0, 0.0, 0.0)
    path: str = ""


@dataclass
class AckermannVanDenBogert2010Force:
    """StationPlaneContactForce.h AckermannVanDenBogert2010Force (properties
    and defaults of its constructProperties): compliant contact of a station
    with the ground plane y = 0, friction along ground x."""
    name: str
    station: str
    stiffness: float = 5e7
    dissipation: float = 1.0
    friction_coefficient: float = 1.0
    tangent_velocity_scaling_factor: float = 0.05
    path: str = ""
    kind = abi.MH_EXT_CONTACT_ACKERMANN_VAN_DEN_BOGERT

    def parameters(self) -> List[float]:
        return [float(self.stiffness), float(self.dissipation), float(self.friction_coefficient),
                float(self.tangent_velocity_scaling_factor), 0.0]


@dataclass
class EspositoMiller2018Force:
    """StationPlaneContactForce.h EspositoMiller2018Force: the smooth
    in / out-of-contact transition with the spring's resting length
    ``depth_offset``."""
    name: str
    station: str
    stiffness: float = 2.0e6
    dissipation: float = 1.0
    friction_coefficient: float = 1.0
    tangent_velocity_scaling_factor: float = 0.05
    depth_offset: float = 0.001
    path: str = ""
    kind = abi.MH_EXT_CONTACT_ESPOSITO_MILLER

    def parameters(self) -> List[float]:
        return [float(self.stiffness), float(self.dissipation), float(self.friction_coefficient),
                float(self.tangent_velocity_scaling_factor), float(self.depth_offset)]


@dataclass
class MeyerFregly2016Force:
    """StationPlaneContactForce.h MeyerFregly2016Force (the friction
    coefficient is fixed at 1 and the latch velocity at 0.05 m/s there)."""
    name: str
    station: str
    stiffness: float = 1e4
    dissipation: float = 1e-2
    tscale: float = 1.0
    path: str = ""
    kind = abi.MH_EXT_CONTACT_MEYER_FREGLY

    def parameters(self) -> List[float]:
        return [float(self.stiffness), float(self.dissipation), 1.0, 0.05, float(self.tscale)]


CONTACT_FORCE_TYPES = (AckermannVanDenBogert2010Force, EspositoMiller2018Force, MeyerFregly2016Force)


@dataclass
class CoordinateCouplerConstraint:
    """OpenSim CoordinateCouplerConstraint with one independent coordinate:
    q[dependent] = scale_factor * function(q[independent]) (the Simbody
    CoordinateCoupler of OpenSim's CompoundFunction; include/mocohip.h
    mh_constraint).  ``function.coord`` names the independent coordinate."""
    name: str
    dependent: str
    function: Function
    scale_factor: float = 1.0


@dataclass
class Bhargava2004MetabolicsMuscleParameters:
    """Bhargava2004Metabolics_MuscleParameters (Bhargava2004Metabolics.cpp:
    40-70): one muscle of a metabolics component.  ``muscle_mass`` NaN: the
    mass is Fmax / specific_tension * density * optimal_fiber_length."""
    name: str
    muscle_path: str
    ratio_slow_twitch_fibers: float = 0.5
    specific_tension: float = 0.25e6
    density: float = 1059.7
    activation_constant_slow_twitch: float = 40.0
    activation_constant_fast_twitch: float = 133.0
    maintenance_constant_slow_twitch: float = 74.0
    maintenance_constant_fast_twitch: float = 111.0
    muscle_mass: float = math.nan

    def mass(self, muscle: "DeGrooteFregly2016Muscle") -> float:
        if not math.isnan(self.muscle_mass):
            return float(self.muscle_mass)
        return (float(muscle.max_isometric_force) / float(self.specific_tension)) * float(self.density) \
            * float(muscle.optimal_fiber_length)


@dataclass
class Bhargava2004Metabolics:
    """Bhargava2004Metabolics (Moco/Moco/Components/Bhargava2004Metabolics.
    {h,cpp}; properties and defaults of its constructProperties): the metabolic
    rate of a set of muscles, the sum of each muscle's activation, maintenance
    and shortening heat rates and mechanical work rate, plus a basal rate for
    the whole model (include/mocohip.h MH_GOAL_METABOLICS gives the formulas).
    A component of a Model (Model.add_component), path ``/<name>``; its outputs
    (abi.METABOLICS_OUTPUTS) are read by MocoOutputGoal and MocoStudy.analyze."""
    name: str = "metabolics"
    enforce_minimum_heat_rate_per_muscle: bool = True
    use_force_dependent_shortening_prop_constant: bool = False
    basal_coefficient: float = 1.2
    basal_exponent: float = 1.0
    muscle_effort_scaling_factor: float = 1.0
    include_negative_mechanical_work: bool = True
    forbid_negative_total_power: bool = True
    use_smoothing: bool = False
    smoothing_type: str = "tanh"
    velocity_smoothing: float = 10.0
    power_smoothing: float = 10.0
    heat_rate_smoothing: float = 10.0
    muscles: List[Bhargava2004MetabolicsMuscleParameters] = field(default_factory=list)

    @property
    def path(self) -> str:
        return "/" + self.name

    def add_muscle(self, name: str, muscle_path: str, ratio_slow_twitch_fibers: float = 0.5,
                   specific_tension: float = 0.25e6, density: float = 1059.7,
                   activation_constant_slow_twitch: float = 40.0, activation_constant_fast_twitch: float = 133.0,
                   maintenance_constant_slow_twitch: float = 74.0, maintenance_constant_fast_twitch: float = 111.0,
                   muscle_mass: float = math.nan):
        """Bhargava2004Metabolics::addMuscle: ``muscle_path`` is the path (or
        the name) of a DeGrooteFregly2016Muscle of the model."""
        mp = Bhargava2004MetabolicsMuscleParameters(
            name, muscle_path, ratio_slow_twitch_fibers, specific_tension, density, activation_constant_slow_twitch,
            activation_constant_fast_twitch, maintenance_constant_slow_twitch, maintenance_constant_fast_twitch,
            muscle_mass)
        self.muscles.append(mp)
        return mp

    def muscle_index(self, model: "Model", mp: Bhargava2004MetabolicsMuscleParameters) -> int:
        """The model's muscle that ``mp`` names; ValueError for a path that
        names none, or an actuator that is no DeGrooteFregly2016Muscle."""
        for i, mu in enumerate(model.muscles):
            if mp.muscle_path in (mu.path, mu.name):
                return i
        other = next((a for a in model.actuators if mp.muscle_path in (getattr(a, "path", None), a.name)), None)
        if other is not None:
            raise ValueError(f"Bhargava2004Metabolics '{self.name}': muscle '{mp.name}': '{mp.muscle_path}' is a "
                             f"{type(other).__name__}, not a DeGrooteFregly2016Muscle")
        raise ValueError(f"Bhargava2004Metabolics '{self.name}': muscle '{mp.name}': no muscle '{mp.muscle_path}' "
                         "in the model")

    def check(self, model: "Model"):
        """ValueError naming the offender: an unknown muscle path, a muscle
        that is no DeGrooteFregly2016Muscle, a name used twice, a ratio outside
        [0, 1], a mass <= 0, a smoothing value <= 0, an unknown smoothing
        type."""
        me = f"Bhargava2004Metabolics '{self.name}'"
        if self.smoothing_type not in ("tanh", "huber"):
            raise ValueError(f"{me}: unknown smoothing_type '{self.smoothing_type}' (tanh or huber)")
        for prop in ("velocity_smoothing", "power_smoothing", "heat_rate_smoothing"):
            if not float(getattr(self, prop)) > 0.0:
                raise ValueError(f"{me}: {prop} = {getattr(self, prop)} is not positive")
        if not self.muscles:
            raise ValueError(f"{me}: no muscles")
        seen = set()
        for mp in self.muscles:
            if mp.name in seen:
                raise ValueError(f"{me}: muscle name '{mp.name}' is used twice")
            seen.add(mp.name)
            im = self.muscle_index(model, mp)
            if not 0.0 <= float(mp.ratio_slow_twitch_fibers) <= 1.0:
                raise ValueError(f"{me}: muscle '{mp.name}': ratio_slow_twitch_fibers = "
                                 f"{mp.ratio_slow_twitch_fibers} is outside [0, 1]")
            if not mp.mass(model.muscles[im]) > 0.0:
                raise ValueError(f"{me}: muscle '{mp.name}': muscle mass {mp.mass(model.muscles[im])} is not positive")

    def flags(self) -> int:
        """The option flags of include/mocohip.h MH_GOAL_METABOLICS."""
        return ((1 if self.use_smoothing else 0) | (2 if self.use_smoothing and self.smoothing_type == "huber" else 0)
                | (4 if self.use_force_dependent_shortening_prop_constant else 0)
                | (8 if self.include_negative_mechanical_work else 0)
                | (16 if self.forbid_negative_total_power else 0)
                | (32 if self.enforce_minimum_heat_rate_per_muscle else 0))

    def term_block(self, model: "Model", output: int = 0, channel: int = -1, divisor: float = 1.0):
        """(index, column, weight) lists: the component as a goal of kind
        MH_GOAL_METABOLICS carries it (include/mocohip.h), the muscle masses and
        the basal rate formed here."""
        self.check(model)
        total_mass = 0.0
        for body in model.bodies.values():
            total_mass += float(body.mass)
        basal = float(self.basal_coefficient) * total_mass ** float(self.basal_exponent)
        idx = [self.flags(), 0, 0, 0, 0, 0]
        col = [int(output), int(channel), 0, 0, 0, 0]
        w = [float(divisor), basal, float(self.muscle_effort_scaling_factor), float(self.velocity_smoothing),
             float(self.power_smoothing), float(self.heat_rate_smoothing)]
        for mp in self.muscles:
            im = self.muscle_index(model, mp)
            idx += [im, 0, 0, 0, 0, 0]
            col += [0] * 6
            w += [mp.mass(model.muscles[im]), float(mp.ratio_slow_twitch_fibers),
                  float(mp.activation_constant_slow_twitch), float(mp.activation_constant_fast_twitch),
                  float(mp.maintenance_constant_slow_twitch), float(mp.maintenance_constant_fast_twitch)]
        return idx, col, w


class Model:
    def __init__(self, name: str = "model", gravity=(0, -9.80665, 0)):
        self.components: List[Bhargava2004Metabolics] = []
        self.name = name
        self.gravity = tuple(float(g) for g in gravity)
        self.bodies: Dict[str, Body] = {}
        self.joints: List[Joint] = []
        self.muscles: List[DeGrooteFregly2016Muscle] = []
        self.actuators: List[object] = []       # force-set order
        self.tables: Dict[str, DataTable] = {}
        self.external_forces: List[ExternalForce] = []
        self.markers: Dict[str, Marker] = {}    # by path
        self.constraints: List[CoordinateCouplerConstraint] = []   # enabled ones
        self.wraps: Dict[str, WrapCylinder] = {}
        self.springs: List[SpringGeneralizedForce] = []
        self.offset_frames: Dict[str, OffsetFrame] = {}   # by path
        self.stations: Dict[str, Station] = {}  # by path
        self.contact_forces: List[object] = []  # the StationPlaneContactForce classes, in the order added

    # building ---------------------------------------------------------------
    def add_body(self, body: Body):
        self.bodies[body.name] = body
        return body

    def add_joint(self, joint: Joint):
        for c in joint.coordinates:
            if not c.path:
                c.path = f"/jointset/{joint.name}/{c.name}"
        self.joints.append(joint)
        return joint

    def add_muscle(self, m: DeGrooteFregly2016Muscle):
        if not m.path:
            m.path = f"/forceset/{m.name}"
        self.muscles.append(m)
        self.actuators.append(m)
        return m

    def add_coordinate_actuator(self, a: CoordinateActuator):
        if not a.path:
            a.path = f"/forceset/{a.name}"
        self.actuators.append(a)
        return a

    def add_spring(self, f: SpringGeneralizedForce):
        if not f.path:
            f.path = f"/forceset/{f.name}"
        self.springs.append(f)
        return f

    def add_table(self, t: DataTable):
        self.tables[t.name] = t
        return t

    def add_external_force(self, e: ExternalForce):
        self.external_forces.append(e)
        return e

    def add_station(self, st: Station):
        if st.body not in self.bodies:
            raise ValueError(f"station '{st.name}': no body '{st.body}'")
        if not st.path:
            st.path = "/" + st.name
        self.stations[st.path] = st
        return st

    def find_station(self, path: str) -> Optional[Station]:
        """The station with that path (``/<name>``, ``/componentset/<name>``
        or ``/bodyset/<body>/<name>``) or name; None when there is none."""
        for st in self.stations.values():
            if path in (st.path, st.name, "/componentset/" + st.name, f"/bodyset/{st.body}/{st.name}"):
                return st
        return None

    def add_contact_force(self, f):
        """A StationPlaneContactForce (AckermannVanDenBogert2010Force,
        EspositoMiller2018Force or MeyerFregly2016Force) on a station of the
        model.  ValueError for an unknown station, a name used twice, a
        non-positive tangent velocity scaling factor or a negative
        depth_offset."""
        if not isinstance(f, CONTACT_FORCE_TYPES):
            raise TypeError(f"not a station-plane contact force: {type(f).__name__}")
        if self.find_station(f.station) is None:
            raise ValueError(f"contact force '{f.name}': no station '{f.station}' in the model")
        if any(g.name == f.name for g in self.contact_forces):
            raise ValueError(f"contact force name '{f.name}' is used twice")
        if not isinstance(f, MeyerFregly2016Force) and not float(f.tangent_velocity_scaling_factor) > 0.0:
            raise ValueError(f"contact force '{f.name}': tangent_velocity_scaling_factor = "
                             f"{f.tangent_velocity_scaling_factor} is not positive")
        if isinstance(f, EspositoMiller2018Force) and not float(f.depth_offset) >= 0.0:
            raise ValueError(f"contact force '{f.name}': depth_offset = {f.depth_offset} is negative")
        if not f.path:
            f.path = f"/forceset/{f.name}"
        self.contact_forces.append(f)
        return f

    def find_contact_force(self, path: str):
        """(index among the contact forces, force) by path or name; None when
        there is none."""
        for i, f in enumerate(self.contact_forces):
            if path in (f.path, f.name, "/" + f.name):
                return i, f
        return None

    def add_constraint(self, k: CoordinateCouplerConstraint):
        self.constraints.append(k)
        return k

    def add_wrap(self, w: WrapCylinder):
        self.wraps[w.name] = w
        return w

    def add_component(self, component: "Bhargava2004Metabolics"):
        """Model::addComponent for a Bhargava2004Metabolics: its path is
        ``/<name>`` (``/componentset/<name>`` is accepted too).  The muscles it
        names must be in the model already."""
        if any(c.name == component.name for c in self.components):
            raise ValueError(f"component name '{component.name}' is used twice")
        component.check(self)
        self.components.append(component)
        return component

    def find_component(self, path: str):
        """The component with path ``/<name>`` or ``/componentset/<name>``
        (None: there is none)."""
        for c in self.components:
            if path in (c.path, "/componentset/" + c.name):
                return c
        return None

    def replace_joints_with_welds(self, names: Sequence[str]):
        """ModOpReplaceJointsWithWelds (ModelFactory::replaceJointWithWeldJoint,
        Moco/Moco/ModelOperators.h, ModelFactory.cpp): each named joint becomes
        a WeldJoint with the same parent / child frames; its coordinates, and
        the actuators on them, are removed."""
        gone = set()
        for j in self.joints:
            if j.name in names:
                gone.update(c.name for c in j.coordinates)
                j.coordinates = []
                j.axes = []
        missing = set(names) - {j.name for j in self.joints}
        if missing:
            raise ValueError(f"no joints {sorted(missing)}")
        for m in self.muscles:
            for p in m.points:
                for f in (p.fx, p.fy, p.fz):
                    if f is not None and f.coord in gone:
                        raise NotImplementedError(f"{m.name}: moving point on welded {f.coord}")
                if p.coord in gone:
                    raise NotImplementedError(f"{m.name}: conditional point on welded {p.coord}")
        self.actuators = [a for a in self.actuators
                          if not (isinstance(a, CoordinateActuator) and a.coordinate in gone)]

    def add_marker(self, mk: Marker):
        if not mk.path:
            mk.path = f"/markerset/{mk.name}"
        self.markers[mk.path] = mk
        return mk

    def add_offset_frame(self, name: str, body: str, translation=(0.0, 0.0, 0.0),
                         orientation=(0.0, 0.0, 0.0)) -> OffsetFrame:
        if body != "ground" and body not in self.bodies:
            raise ValueError(f"offset frame '{name}': no body '{body}'")
        path = f"/ground/{name}" if body == "ground" else f"/bodyset/{body}/{name}"
        fr = OffsetFrame(name, body, tuple(float(v) for v in translation), path,
                         tuple(float(v) for v in orientation))
        self.offset_frames[path] = fr
        return fr

    def find_frame(self, path: str):
        """(body name or "ground", location in that body) of the Frame at
        ``path``: /ground, /bodyset/<body>, a body name, or a registered
        offset frame (by path or name); None when there is none."""
        if path in ("/ground", "ground"):
            return "ground", (0.0, 0.0, 0.0)
        for b in self.bodies:
            if path in (b, "/bodyset/" + b):
                return b, (0.0, 0.0, 0.0)
        for fr in self.offset_frames.values():
            if path in (fr.path, fr.name):
                return fr.body, tuple(fr.translation)
        return None

    def find_frame_orientation(self, path: str) -> Optional[np.ndarray]:
        """R_BO, the orientation in its body of the Frame at ``path`` (what
        find_frame resolves): body_fixed_xyz of an offset frame's angles, the
        identity for ground and a body; None when there is no such frame."""
        if self.find_frame(path) is None:
            return None
        if path not in ("/ground", "ground") and not any(path in (b, "/bodyset/" + b) for b in self.bodies):
            for fr in self.offset_frames.values():
                if path in (fr.path, fr.name):
                    return body_fixed_xyz(fr.orientation)
        return np.eye(3)

    def frame_pose_in_ground(self, path: str, coordinates: Dict[str, float]):
        """(position of the origin, rotation) in ground of the Frame at
        ``path`` at the given coordinate values (as marker_locations_in_ground
        takes them): Frame::getPositionInGround / getRotationInGround.  For
        frame-tracking references computed from states, and for synthesizing
        data (configs.py); not on the hot path."""
        fr = self.find_frame(path)
        if fr is None:
            raise ValueError(f"no frame '{path}' in the model")
        X = self._body_transforms_in_ground(coordinates)[fr[0]]
        return (X @ np.append(np.asarray(fr[1], float), 1.0))[:3], X[:3, :3] @ self.find_frame_orientation(path)

    def frame_angular_velocity_in_ground(self, path: str, coordinates: Dict[str, float],
                                         speeds: Dict[str, float]) -> np.ndarray:
        """The angular velocity in ground, expressed in ground, of the Frame
        at ``path`` at the given coordinate values and speeds (both by
        coordinate name; a missing speed is 0):
        Frame::getAngularVelocityInGround.  A frame welded to a body has the
        body's angular velocity; ground's is 0.  For angular-velocity
        references computed from states, and for synthesizing data; not on
        the hot path."""
        fr = self.find_frame(path)
        if fr is None:
            raise ValueError(f"no frame '{path}' in the model")
        return self._body_angular_velocities_in_ground(coordinates, speeds)[fr[0]]

    def _body_angular_velocities_in_ground(self, coordinates: Dict[str, float],
                                           speeds: Dict[str, float]) -> Dict[str, np.ndarray]:
        """Every body's angular velocity in ground: along the tree, the
        parent's plus, for each rotation axis of the joint that a coordinate
        moves, (the axis in ground, after the joint's earlier rotations) x
        (the axis function's slope) x (the coordinate's speed)."""
        from .splines import SimmSpline
        X_G = self._body_transforms_in_ground(coordinates)
        qdefault = {c.name: c.default_value for c in self.coordinates()}
        w_G = {"ground": np.zeros(3)}
        for j in self.tree_order():
            R_GF = X_G[j.parent][:3, :3] @ body_fixed_xyz(j.orient_in_parent)
            R_cur, w = np.eye(3), w_G[j.parent].copy()
            for ax in j.axes:
                if ax.type != abi.MH_AXIS_ROTATION:
                    continue
                f, a = ax.func, np.asarray(unit3(ax.dir))
                if f.kind == abi.MH_FN_CONSTANT:
                    t = f.a
                else:
                    q = float(coordinates.get(f.coord, qdefault.get(f.coord, 0.0)))
                    if f.kind == abi.MH_FN_LINEAR:
                        t, slope = f.scale * (f.a * q + f.b), f.scale * f.a
                    else:
                        sp = SimmSpline(f.x, f.y)
                        t, slope = f.scale * float(sp(q)), f.scale * float(sp(q, deriv=1))
                    w = w + (R_GF @ R_cur @ a) * (slope * float(speeds.get(f.coord, 0.0)))
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                R_cur = R_cur @ (np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K))
            w_G[j.child] = w
        return w_G

    def marker_locations_in_ground(self, coordinates: Dict[str, float]) -> Dict[str, np.ndarray]:
        """Every marker's location in ground (by marker path) at the given
        coordinate values (by coordinate name; a missing one is at its
        default).  For synthesizing marker data from coordinate trajectories
        (configs.py); not on the hot path."""
        X_G = self._body_transforms_in_ground(coordinates)
        return {path: (X_G[mk.body] @ np.append(np.asarray(mk.location, float), 1.0))[:3]
                for path, mk in self.markers.items()}

    def _body_transforms_in_ground(self, coordinates: Dict[str, float]) -> Dict[str, np.ndarray]:
        """Every body's transform in ground (and ground's) at the given
        coordinate values: the position part of the forward kinematics --
        parent pose x joint frames x axis functions -- in NumPy, as 4x4
        transforms."""
        from .splines import SimmSpline

        def value(f: Function) -> float:
            if f.kind == abi.MH_FN_CONSTANT:
                return f.a
            q = float(coordinates.get(f.coord, qdefault.get(f.coord, 0.0)))
            if f.kind == abi.MH_FN_LINEAR:
                return f.scale * (f.a * q + f.b)
            return f.scale * float(SimmSpline(f.x, f.y)(q))

        def transform(R=None, p=(0.0, 0.0, 0.0)):
            X = np.eye(4)
            if R is not None:
                X[:3, :3] = R
            X[:3, 3] = p
            return X

        qdefault = {c.name: c.default_value for c in self.coordinates()}
        X_G = {"ground": np.eye(4)}
        for j in self.tree_order():
            X_FM = np.eye(4)
            for ax in j.axes:      # translations first, then the rotations in order
                if ax.type == abi.MH_AXIS_TRANSLATION:
                    X_FM = X_FM @ transform(p=value(ax.func) * np.asarray(unit3(ax.dir)))
            for ax in j.axes:
                if ax.type == abi.MH_AXIS_ROTATION:
                    a, t = np.asarray(unit3(ax.dir)), value(ax.func)
                    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                    X_FM = X_FM @ transform(np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K))
            X_PF = transform(body_fixed_xyz(j.orient_in_parent), j.loc_in_parent)
            X_BM = transform(body_fixed_xyz(j.orient_in_child), j.loc_in_child)
            X_G[j.child] = X_G[j.parent] @ X_PF @ X_FM @ np.linalg.inv(X_BM)
        return X_G

    # ordering ---------------------------------------------------------------
    def tree_order(self) -> List[Joint]:
        """Joints in Simbody mobilized-body order: breadth-first by tree
        level, model joint order within a level (MultibodyGraphMaker)."""
        order: List[Joint] = []
        placed = {"ground"}
        remaining = list(self.joints)
        while remaining:
            level = [j for j in remaining if j.parent in placed]
            if not level:
                raise ValueError("model graph is not a tree rooted at ground")
            for j in level:
                order.append(j)
            for j in level:
                placed.add(j.child)
            remaining = [j for j in remaining if j not in level]
        return order

    def coordinates(self) -> List[Coordinate]:
        return [c for j in self.tree_order() for c in j.coordinates]

    def coordinate_index(self) -> Dict[str, int]:
        return {c.name: i for i, c in enumerate(self.coordinates())}

    def state_names(self) -> List[str]:
        qs = self.coordinates()
        names = [c.path + "/value" for c in qs] + [c.path + "/speed" for c in qs]
        for m in self.muscles:
            if not m.ignore_activation_dynamics:
                names.append(m.path + "/activation")
            if not m.ignore_tendon_compliance:
                names.append(m.path + "/normalized_tendon_force")
        return names

    def control_names(self) -> List[str]:
        return [a.path for a in self.actuators]

    # lowering ---------------------------------------------------------------
    def compile(self, extra_tables: Sequence[DataTable] = ()) -> "CompiledModel":
        """Lower to mh_model.  ``extra_tables`` (problem-level functions of
        time, e.g. path-constraint bounds) are appended after the model's
        own tables, which keep their indices."""
        return CompiledModel(self, extra_tables)


def _arr(struct_type, items):
    n = len(items)
    arr = (struct_type * max(n, 1))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


class CompiledModel:
    """Owns the C arrays that back an mh_model."""

    def __init__(self, model: Model, extra_tables: Sequence[DataTable] = ()):
        self.model = model
        qidx = model.coordinate_index()
        self.qidx = qidx
        joints = model.tree_order()
        body_index = {"ground": -1}
        for i, j in enumerate(joints):
            body_index[j.child] = i
        self.body_index = body_index
        funcs: List[abi.mh_function] = []
        knot_x: List[float] = []
        knot_y: List[float] = []

        def add_function(f: Optional[Function]) -> int:
            if f is None:
                return -1
            fs = abi.mh_function()
            fs.kind = f.kind
            fs.coord = qidx[f.coord] if f.coord is not None and f.kind != abi.MH_FN_CONSTANT else -1
            fs.a, fs.b, fs.scale = f.a, f.b, f.scale
            if f.kind == abi.MH_FN_SIMMSPLINE:
                fs.knot_begin = len(knot_x)
                fs.knot_count = len(f.x)
                knot_x.extend(f.x)
                knot_y.extend(f.y)
            funcs.append(fs)
            return len(funcs) - 1

        bodies, axes = [], []
        for j in joints:
            B = model.bodies[j.child]
            b = abi.mh_body()
            b.parent = body_index[j.parent]
            b.mass = B.mass
            b.com[:] = list(map(float, B.com))
            b.inertia[:] = list(map(float, B.inertia))
            R_PF = body_fixed_xyz(j.orient_in_parent)
            R_BM = body_fixed_xyz(j.orient_in_child)
            b.R_PF[:] = R_PF.reshape(-1).tolist()
            b.p_PF[:] = list(map(float, j.loc_in_parent))
            b.R_BM[:] = R_BM.reshape(-1).tolist()
            b.p_BM[:] = list(map(float, j.loc_in_child))
            b.axis_begin = len(axes)
            for ax in j.axes:
                a = abi.mh_axis()
                a.type = ax.type
                a.dir[:] = unit3(ax.dir)
                a.func = add_function(ax.func)
                axes.append(a)
            b.axis_count = len(axes) - b.axis_begin
            bodies.append(b)

        points, muscles = [], []
        for m in model.muscles:
            ms = abi.mh_muscle()
            ms.point_begin = len(points)
            for p in m.points:
                ps = abi.mh_path_point()
                ps.kind = p.kind
                ps.body = body_index[p.body]
                ps.loc[:] = list(map(float, p.loc))
                ps.coord = qidx[p.coord] if p.coord is not None else -1
                ps.range[:] = list(map(float, p.range))
                ps.fx = add_function(p.fx)
                ps.fy = add_function(p.fy)
                ps.fz = add_function(p.fz)
                points.append(ps)
            ms.point_count = len(points) - ms.point_begin
            ms.ignore_activation_dynamics = int(m.ignore_activation_dynamics)
            ms.ignore_tendon_compliance = int(m.ignore_tendon_compliance)
            ms.ignore_passive_fiber_force = int(m.ignore_passive_fiber_force)
            ms.tendon_dynamics_implicit = int(
                m.tendon_compliance_dynamics_mode == "implicit")
            for k in ("max_isometric_force", "optimal_fiber_length",
                      "tendon_slack_length", "pennation_angle_at_optimal",
                      "max_contraction_velocity", "activation_time_constant",
                      "deactivation_time_constant", "fiber_damping",
                      "passive_fiber_strain_at_one_norm_force",
                      "tendon_strain_at_one_norm_force",
                      "active_force_width_scale"):
                setattr(ms, k, float(getattr(m, k)))
            muscles.append(ms)

        # wrap surfaces (in model order) and the PathWrap list per muscle
        wraps, pathwraps = [], []
        wrap_index = {}
        for w in model.wraps.values():
            if not w.active:
                continue
            ws = abi.mh_wrap_object()
            ws.kind = abi.MH_WRAP_CYLINDER
            ws.body = body_index[w.body]
            ws.wrap_axis, ws.wrap_sign = quadrant_axis_sign(w.quadrant)
            ws.R_BW[:] = body_fixed_xyz(w.xyz_body_rotation).reshape(-1).tolist()
            ws.p_BW[:] = list(map(float, w.translation))
            ws.radius = float(w.radius)
            ws.length = float(w.length)
            wrap_index[w.name] = len(wraps)
            wraps.append(ws)
        for im, m in enumerate(model.muscles):
            for (wname, r0, r1) in m.path_wraps:
                if wname not in wrap_index:
                    if wname in model.wraps:
                        continue        # inactive wrap object
                    raise ValueError(f"{m.name}: unknown wrap object {wname}")
                pw = abi.mh_path_wrap()
                pw.muscle, pw.wrap = im, wrap_index[wname]
                pw.range_begin, pw.range_end = int(r0), int(r1)
                pathwraps.append(pw)
        self._wraps = _arr(abi.mh_wrap_object, wraps)
        self._pathwraps = _arr(abi.mh_path_wrap, pathwraps)

        muscle_index = {id(m): i for i, m in enumerate(model.muscles)}
        acts = []
        for a in model.actuators:
            s = abi.mh_actuator()
            if isinstance(a, DeGrooteFregly2016Muscle):
                s.kind = abi.MH_ACT_MUSCLE
                s.target = muscle_index[id(a)]
                s.optimal_force = 1.0
            else:
                s.kind = abi.MH_ACT_COORDINATE
                s.target = qidx[a.coordinate]
                s.optimal_force = float(a.optimal_force)
            acts.append(s)

        # data tables -> piecewise polynomials
        tables, breaks, coefs = [], [], []
        self.table_index: Dict[str, int] = {}
        self.table_columns: Dict[str, List[str]] = {}
        all_tables = list(model.tables.items()) + [(t.name, t) for t in extra_tables]
        for name, t in all_tables:
            cols = list(t.columns.keys())
            if t.ppoly is not None:
                br, cf = t.ppoly
            else:
                br, cf = gcv_interpolating_ppoly(
                    np.asarray(t.times, float),
                    np.stack([np.asarray(t.columns[c], float) for c in cols], 1),
                    t.degree)
            ts = abi.mh_table()
            ts.nseg = len(br) - 1
            ts.degree = cf.shape[-1] - 1
            ts.ncol = len(cols)
            ts.break_begin = len(breaks)
            ts.coef_begin = len(coefs)
            breaks.extend(br.tolist())
            coefs.extend(cf.reshape(-1).tolist())
            self.table_index[name] = len(tables)
            self.table_columns[name] = cols
            tables.append(ts)

        ext = []
        for e in model.external_forces:
            es = abi.mh_external_force()
            es.body = body_index[e.body]
            es.table = self.table_index[e.table]
            cols = self.table_columns[e.table]

            def col3(ident):
                if ident is None:
                    return -1
                i = cols.index(ident + "x")
                assert cols[i + 1] == ident + "y" and cols[i + 2] == ident + "z"
                return i
            es.force_col = col3(e.force_identifier)
            es.point_col = col3(e.point_identifier)
            es.torque_col = col3(e.torque_identifier)
            ext.append(es)

        # station-plane contact forces: records after the table-driven ones,
        # parameter blocks after all table coefficients (include/mocohip.h)
        for f in model.contact_forces:
            st = model.find_station(f.station)
            es = abi.mh_external_force()
            es.body = body_index[st.body]
            es.table = es.point_col = es.torque_col = -1
            es.force_col = len(coefs)
            es.kind = f.kind
            coefs.extend([float(v) for v in st.location] + f.parameters())
            ext.append(es)
        self.ncontacts = len(model.contact_forces)

        self._bodies = _arr(abi.mh_body, bodies)
        self._axes = _arr(abi.mh_axis, axes)
        self._funcs = _arr(abi.mh_function, funcs)
        self._kx = np.ascontiguousarray(knot_x + [0.0], float)
        self._ky = np.ascontiguousarray(knot_y + [0.0], float)
        self._muscles = _arr(abi.mh_muscle, muscles)
        self._points = _arr(abi.mh_path_point, points)
        self._acts = _arr(abi.mh_actuator, acts)
        self._tables = _arr(abi.mh_table, tables)
        self._breaks = np.ascontiguousarray(breaks + [0.0], float)
        self._coefs = np.ascontiguousarray(coefs + [0.0], float)
        self._ext = _arr(abi.mh_external_force, ext)
        # kinematic constraints: their functions after every other function
        # (models without constraints keep their function list and hash)
        kcs = []
        for k in model.constraints:
            if k.function.kind == abi.MH_FN_CONSTANT or k.function.coord is None:
                raise ValueError(f"constraint {k.name}: needs a function of the independent coordinate")
            ks = abi.mh_constraint()
            ks.kind = abi.MH_KC_COORDINATE_COUPLER
            ks.dependent = qidx[k.dependent]
            ks.func = add_function(k.function)
            ks.scale = float(k.scale_factor)
            kcs.append(ks)
        self._funcs = _arr(abi.mh_function, funcs)
        self._kx = np.ascontiguousarray(knot_x + [0.0], float)
        self._ky = np.ascontiguousarray(knot_y + [0.0], float)
        self._kcs = _arr(abi.mh_constraint, kcs)
        springs = []
        for f in model.springs:
            ss = abi.mh_spring()
            ss.coord = qidx[f.coordinate]
            ss.stiffness, ss.rest_length, ss.viscosity = float(f.stiffness), float(f.rest_length), float(f.viscosity)
            springs.append(ss)
        self._springs = _arr(abi.mh_spring, springs)

        mm = abi.mh_model()
        mm.nq = len(qidx)
        mm.nbodies = len(bodies)
        mm.naxes = len(axes)
        mm.nfunctions = len(funcs)
        mm.nknots = len(knot_x)
        mm.nconstraints = len(kcs)
        mm.constraints = self._kcs
        mm.nmuscles = len(muscles)
        mm.npoints = len(points)
        mm.nactuators = len(acts)
        mm.ntables = len(tables)
        mm.nbreaks = len(breaks)
        mm.ncoefs = len(coefs)
        mm.nexternal = len(ext)
        mm.gravity[:] = list(model.gravity)
        mm.bodies = self._bodies
        mm.axes = self._axes
        mm.functions = self._funcs
        mm.knot_x = abi.dptr(self._kx)
        mm.knot_y = abi.dptr(self._ky)
        mm.muscles = self._muscles
        mm.points = self._points
        mm.actuators = self._acts
        mm.tables = self._tables
        mm.table_breaks = abi.dptr(self._breaks)
        mm.table_coefs = abi.dptr(self._coefs)
        mm.external = self._ext
        mm.nwraps = len(wraps)
        mm.npathwraps = len(pathwraps)
        mm.wraps = self._wraps
        mm.pathwraps = self._pathwraps
        mm.nsprings = len(springs)
        mm.springs = self._springs
        self.struct = mm
        self.nq = mm.nq
        self.state_names = model.state_names()
        self.control_names = model.control_names()


# --------------------------------------------------------------------------
# JSON round trip (committed model data under mocohip/data/).
# --------------------------------------------------------------------------
def _fn_to(f: Optional[Function]):
    if f is None:
        return None
    return {"kind": f.kind, "coord": f.coord, "a": f.a, "b": f.b,
            "scale": f.scale, "x": list(f.x), "y": list(f.y)}


def _fn_from(d) -> Optional[Function]:
    if d is None:
        return None
    return Function(d["kind"], d["coord"], d["a"], d["b"], d["scale"],
                    d["x"], d["y"])


def model_to_dict(m: Model) -> dict:
    return {
        "name": m.name, "gravity": list(m.gravity),
        "bodies": [{"name": b.name, "mass": b.mass, "com": list(b.com),
                    "inertia": list(b.inertia)} for b in m.bodies.values()],
        "joints": [{
            "name": j.name, "parent": j.parent, "child": j.child,
            "coordinates": [{"name": c.name, "range": list(c.range),
                             "motion_type": c.motion_type,
                             "default_value": c.default_value, "path": c.path}
                            for c in j.coordinates],
            "axes": [{"type": a.type, "dir": list(a.dir), "func": _fn_to(a.func)}
                     for a in j.axes],
            "loc_in_parent": list(j.loc_in_parent),
            "orient_in_parent": list(j.orient_in_parent),
            "loc_in_child": list(j.loc_in_child),
            "orient_in_child": list(j.orient_in_child)} for j in m.joints],
        "actuators": [
            ({"type": "muscle", **{k: getattr(a, k) for k in a.__dataclass_fields__
                                    if k != "points"},
              "points": [{"body": p.body, "loc": list(p.loc), "kind": p.kind,
                          "coord": p.coord, "range": list(p.range),
                          "fx": _fn_to(p.fx), "fy": _fn_to(p.fy),
                          "fz": _fn_to(p.fz), "name": p.name} for p in a.points]}
             if isinstance(a, DeGrooteFregly2016Muscle) else
             {"type": "coordinate_actuator", "name": a.name,
              "coordinate": a.coordinate, "optimal_force": a.optimal_force,
              "min_control": a.min_control, "max_control": a.max_control,
              "path": a.path})
            for a in m.actuators],
        "markers": [{"name": k.name, "body": k.body, "location": list(k.location), "path": k.path}
                    for k in m.markers.values()],
        "wraps": [{"name": w.name, "body": w.body, "radius": w.radius, "length": w.length,
                   "xyz_body_rotation": list(w.xyz_body_rotation),
                   "translation": list(w.translation), "quadrant": w.quadrant,
                   "active": w.active} for w in m.wraps.values()],
        "constraints": [{"name": k.name, "dependent": k.dependent, "function": _fn_to(k.function),
                         "scale_factor": k.scale_factor} for k in m.constraints],
        "springs": [{"name": f.name, "coordinate": f.coordinate, "stiffness": f.stiffness,
                     "rest_length": f.rest_length, "viscosity": f.viscosity, "path": f.path}
                    for f in m.springs],
        **({"stations": [{"name": t.name, "body": t.body, "location": list(t.location), "path": t.path}
                         for t in m.stations.values()]} if m.stations else {}),
        **({"contact_forces": [{"type": type(f).__name__,
                                **{k: getattr(f, k) for k in f.__dataclass_fields__}}
                               for f in m.contact_forces]} if m.contact_forces else {}),
        **({"offset_frames": [{"name": f.name, "body": f.body, "translation": list(f.translation),
                               **({"orientation": list(f.orientation)} if f.oriented() else {})}
                              for f in m.offset_frames.values()]} if m.offset_frames else {}),
    }


def model_from_dict(d: dict) -> Model:
    m = Model(d["name"], tuple(d["gravity"]))
    for b in d["bodies"]:
        m.add_body(Body(b["name"], b["mass"], tuple(b["com"]), tuple(b["inertia"])))
    for j in d["joints"]:
        coords = [Coordinate(c["name"], tuple(c["range"]), c["motion_type"],
                             c["default_value"], c["path"]) for c in j["coordinates"]]
        axes = [Axis(a["type"], tuple(a["dir"]), _fn_from(a["func"])) for a in j["axes"]]
        m.add_joint(Joint(j["name"], j["parent"], j["child"], coords, axes,
                          tuple(j["loc_in_parent"]), tuple(j["orient_in_parent"]),
                          tuple(j["loc_in_child"]), tuple(j["orient_in_child"])))
    for a in d["actuators"]:
        if a["type"] == "muscle":
            pts = [PathPoint(p["body"], tuple(p["loc"]), p["kind"], p["coord"],
                             tuple(p["range"]), _fn_from(p["fx"]), _fn_from(p["fy"]),
                             _fn_from(p["fz"]), p["name"]) for p in a["points"]]
            kw = {k: v for k, v in a.items() if k not in ("type", "points")}
            kw["path_wraps"] = [tuple(w) for w in kw.get("path_wraps", [])]
            m.add_muscle(DeGrooteFregly2016Muscle(points=pts, **kw))
        else:
            m.add_coordinate_actuator(CoordinateActuator(
                a["name"], a["coordinate"], a["optimal_force"], a["min_control"],
                a["max_control"], a["path"]))
    for k in d.get("markers", []):
        m.add_marker(Marker(k["name"], k["body"], tuple(k["location"]), k.get("path", "")))
    for w in d.get("wraps", []):
        m.add_wrap(WrapCylinder(w["name"], w["body"], w["radius"], w["length"],
                                tuple(w["xyz_body_rotation"]), tuple(w["translation"]),
                                w["quadrant"], w["active"]))
    for k in d.get("constraints", []):
        m.add_constraint(CoordinateCouplerConstraint(k["name"], k["dependent"],
                                                     _fn_from(k["function"]), k["scale_factor"]))
    for f in d.get("springs", []):
        m.add_spring(SpringGeneralizedForce(f["name"], f["coordinate"], f["stiffness"], f["rest_length"],
                                            f["viscosity"], f.get("path", "")))
    for t in d.get("stations", []):
        m.add_station(Station(t["name"], t["body"], tuple(t["location"]), t.get("path", "")))
    for f in d.get("contact_forces", []):
        cls = {c.__name__: c for c in CONTACT_FORCE_TYPES}[f["type"]]
        m.add_contact_force(cls(**{k: v for k, v in f.items() if k != "type"}))
    for f in d.get("offset_frames", []):
        m.add_offset_frame(f["name"], f["body"], tuple(f["translation"]), tuple(f.get("orientation", (0.0, 0.0, 0.0))))
    return m
