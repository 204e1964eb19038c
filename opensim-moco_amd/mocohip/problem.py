"""MocoProblem / MocoProblemRep mirror: goals, bounds rules, and lowering of
a problem to the C-ABI ``mh_problem`` struct.

Default-bound rules restate MocoProblemRep::initialize
(Moco/Moco/MocoProblemRep.cpp:306-427) and MocoPhase defaults
(Moco/Moco/MocoProblem.cpp:30-43).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .model import CompiledModel, CoordinateActuator, DataTable, \
    DeGrooteFregly2016Muscle, Model, SpringGeneralizedForce, body_fixed_xyz, unit3
from .splines import gcv_interpolating_ppoly

NAN = float("nan")


@dataclass
class MocoBounds:
    lower: float = NAN
    upper: float = NAN

    @staticmethod
    def of(b) -> "MocoBounds":
        if b is None:
            return MocoBounds()
        if isinstance(b, MocoBounds):
            return b
        if isinstance(b, (int, float)):
            return MocoBounds(float(b), float(b))
        lo, hi = b
        return MocoBounds(float(lo), float(hi))

    def is_set(self) -> bool:
        return not (math.isnan(self.lower) or math.isnan(self.upper))


@dataclass
class MocoVariableInfo:
    bounds: MocoBounds = field(default_factory=MocoBounds)
    initial: MocoBounds = field(default_factory=MocoBounds)
    final: MocoBounds = field(default_factory=MocoBounds)


# ---------------------------------------------------------------- goals ----
@dataclass
class MocoControlGoal:
    """MocoControlGoal (Moco/Moco/MocoGoal/MocoControlGoal.cpp:54-131)."""
    name: str = "control_effort"
    weight: float = 1.0
    exponent: int = 2
    control_weights: Dict[str, float] = field(default_factory=dict)


@dataclass
class MocoStateTrackingGoal:
    """MocoStateTrackingGoal (MocoStateTrackingGoal.cpp:27-117).  The
    reference is a DataTable whose column labels are state paths."""
    name: str = "state_tracking"
    weight: float = 1.0
    reference: Optional[DataTable] = None
    state_weights: Dict[str, float] = field(default_factory=dict)


@dataclass
class MocoFinalTimeGoal:
    name: str = "final_time"
    weight: float = 1.0


@dataclass
class MocoSumSquaredStateGoal:
    name: str = "sum_squared_state"
    weight: float = 1.0
    state_weights: Dict[str, float] = field(default_factory=dict)


@dataclass
class MocoInitialActivationGoal:
    """MocoInitialActivationGoal (Moco/Moco/MocoGoal/MocoInitialActivationGoal.
    {h,cpp}): for every muscle with activation dynamics, the initial
    excitation equals the initial activation.  An endpoint constraint by
    default (getDefaultModeImpl, .h:40-42; MocoGoal.h:254-271 sets the weight
    to 1 in that mode); one equation per muscle in model order
    (initializeOnModelImpl, .cpp:23-39), bounds [0, 0]
    (MocoConstraintInfo.h:44-54)."""
    name: str = "initial_activation"
    mode: str = "endpoint_constraint"
    weight: float = 1.0


@dataclass
class MocoMarkerFinalGoal:
    """MocoMarkerFinalGoal (Moco/Moco/MocoGoal/MocoMarkerFinalGoal.{h,cpp}):
    cost = |location in ground of ``point_name`` at the final state -
    ``reference_location``|^2 (calcGoalImpl, .cpp:29-34; realizes Position
    only, so it depends on the final coordinates), times the weight."""
    name: str = "marker_final"
    weight: float = 1.0
    point_name: str = ""
    reference_location: Sequence[float] = (0.0, 0.0, 0.0)


@dataclass
class MarkersReference:
    """OpenSim::MarkersReference: a table of Vec3 columns labelled by marker
    name or component path (``positions[row][marker][xyz]`` at ``times``) and
    a weight per marker, 1.0 unless set (the MarkersReference constructor's
    default).  ``flatten()`` is TimeSeriesTableVec3::flatten(): the columns
    <label>_1, <label>_2, <label>_3, splined as GCVSplineSet(table) does
    (degree 5).  As for a state-tracking reference, the flattened table is a
    table of the model (Model.add_table) under ``name``."""
    name: str = "markers_reference"
    times: Sequence[float] = ()
    labels: List[str] = field(default_factory=list)
    positions: Optional[np.ndarray] = None
    marker_weights: Dict[str, float] = field(default_factory=dict)
    degree: int = 5

    def set_marker_weight(self, label: str, weight: float):
        self.marker_weights[label] = float(weight)

    def weights(self) -> List[float]:
        """The weights by reference index (MarkersReference::getWeights)."""
        return [float(self.marker_weights.get(n, 1.0)) for n in self.labels]

    def flatten(self) -> DataTable:
        check_redundant_labels(self.labels)
        pos = np.asarray(self.positions, float)
        if pos.shape != (len(self.times), len(self.labels), 3):
            raise ValueError(f"MarkersReference: positions of shape {pos.shape}, expected "
                             f"{(len(self.times), len(self.labels), 3)}")
        cols = {f"{n}_{c + 1}": np.ascontiguousarray(pos[:, i, c])
                for i, n in enumerate(self.labels) for c in range(3)}
        return DataTable(self.name, np.asarray(self.times, float), cols, degree=self.degree)


def check_redundant_labels(labels):
    """checkRedundantLabels (MocoUtilities.cpp:635-640)."""
    srt = sorted(labels)
    for a, b in zip(srt, srt[1:]):
        if a == b:
            raise ValueError(f"Label '{a}' appears more than once.")


@dataclass
class MocoMarkerTrackingGoal:
    """MocoMarkerTrackingGoal (Moco/Moco/MocoGoal/MocoMarkerTrackingGoal.
    {h,cpp}): the integral over the phase of sum_m w_m |location in ground of
    model marker m - reference_m(t)|^2, times the weight.  A reference label
    names a model marker by component path or, failing that, by its name in
    the marker set; a label that names none is an error unless
    ``allow_unused_references`` (initializeOnModelImpl, .cpp:28-83)."""
    name: str = "marker_tracking"
    weight: float = 1.0
    markers_reference: Optional[MarkersReference] = None
    allow_unused_references: bool = False


def rotation_to_quaternion(R) -> np.ndarray:
    """(e0, e1, e2, e3) of the rotation matrix R by the standard four-case
    method: from the trace when it is the largest of (trace, R00, R11, R22),
    else from the largest diagonal entry; canonicalised to e0 >= 0 and
    normalised.  This is Simbody's Rotation::convertRotationToQuaternion as
    recalled -- Simbody is not at hand, so the convention (case order, sign) is
    not pinned against it.  q and -q are the same rotation; e0 >= 0 picks one,
    but near e0 = 0 (a half turn) consecutive rows of a table can still land on
    opposite signs, and the splined, re-normalised quaternion then passes
    through garbage between them.  The reference does not repair such flips
    and neither does this."""
    R = np.asarray(R, float)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= R[0, 0] and tr >= R[1, 1] and tr >= R[2, 2]:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        q = np.array([R[2, 1] - R[1, 2], 1.0 - (tr - 2.0 * R[0, 0]), R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif R[1, 1] >= R[2, 2]:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 - (tr - 2.0 * R[1, 1]), R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 - (tr - 2.0 * R[2, 2])])
    q = q / math.sqrt(float(q @ q))
    return -q if q[0] < 0.0 else q


@dataclass
class FrameReference:
    """A TimeSeriesTableVec3 of frame positions (``values[row][frame][xyz]``)
    or a TimeSeriesTable_<Rotation> of frame rotations in ground
    (``values[row][frame][3][3]``), labelled by frame path."""
    times: Sequence[float] = ()
    labels: List[str] = field(default_factory=list)
    values: Optional[np.ndarray] = None


@dataclass
class _FrameTrackingGoal:
    """What MocoTranslationTrackingGoal and MocoOrientationTrackingGoal share
    (initializeOnModelImpl of either): the reference given as a table of
    frame data or as states, the frame_paths selection, the weights.

    The reference is either ``reference`` (a FrameReference) or
    ``states_reference`` (a DataTable whose labels are state paths; the frame
    data is computed at each row by forward kinematics), never both.  With a
    table, an empty ``frame_paths`` tracks every column and a non-empty one
    selects the named columns -- the documented behaviour; the reference's
    code tests the property the wrong way round.  With states,
    ``frame_paths`` is required.  The flattened table (``reference_table``) is
    a table of the model (Model.add_table) under ``reference_name()``, as a
    marker goal's is."""
    name: str = ""
    weight: float = 1.0
    reference: Optional[FrameReference] = None
    states_reference: Optional[DataTable] = None
    frame_paths: List[str] = field(default_factory=list)
    frame_weights: Dict[str, float] = field(default_factory=dict)
    table_name: str = ""
    degree: int = 5

    WHAT = ""        # "translation" / "rotation", as in the reference's messages
    SUFFIXES = ()

    def set_weight_for_frame(self, frame_path: str, weight: float):
        self.frame_weights[frame_path] = float(weight)

    def weight_for_frame(self, frame_path: str) -> float:
        return float(self.frame_weights.get(frame_path, 1.0))

    def reference_name(self) -> str:
        return self.table_name or f"{self.name}_reference"

    def tracked_frame_paths(self) -> List[str]:
        if self.reference is not None and self.states_reference is not None:
            raise ValueError(f"{type(self).__name__}: a {self.WHAT} reference and a states reference "
                             "cannot both be given")
        if self.reference is not None:
            labels = list(self.reference.labels)
            if not self.frame_paths:
                paths = labels
            else:
                for path in self.frame_paths:
                    if path not in labels:
                        raise ValueError(f"Expected frame_paths to match one of the column labels in the "
                                         f"{self.WHAT} reference, but frame path '{path}' not found in the "
                                         "reference labels.")
                paths = list(self.frame_paths)
        elif self.states_reference is not None:
            if not self.frame_paths:
                raise ValueError("Expected paths in the frame_paths property, but none were found.")
            paths = list(self.frame_paths)
        else:
            raise ValueError(f"{type(self).__name__}: no reference")
        check_redundant_labels(paths)
        return paths

    def _frame_values(self, model: Model, paths: List[str]):
        """times and values[row][frame] (a position or a rotation)."""
        if self.reference is not None:
            vals = np.asarray(self.reference.values, float)
            if vals.shape[:2] != (len(self.reference.times), len(self.reference.labels)):
                raise ValueError(f"{type(self).__name__}: reference values of shape {vals.shape} for "
                                 f"{len(self.reference.times)} rows and {len(self.reference.labels)} labels")
            idx = [self.reference.labels.index(p) for p in paths]
            return np.asarray(self.reference.times, float), vals[:, idx]
        ref = self.states_reference
        states = set()
        for c in model.coordinates():
            states.update((c.path + "/value", c.path + "/speed"))
        for mu in model.muscles:
            states.update((mu.path + "/activation", mu.path + "/normalized_tendon_force"))
        for label in ref.columns:          # checkLabelsMatchModelStates
            if label not in states:
                raise ValueError(f"Expected the provided labels to match the model state names, but label "
                                 f"{label} does not correspond to any model state.")
        bypath = {c.path + "/value": c.name for c in model.coordinates()}
        cols = {bypath[k]: np.asarray(v, float) for k, v in ref.columns.items() if k in bypath}
        vals = self._values_from_states(model, paths, ref, cols)
        return np.asarray(ref.times, float), np.asarray(vals, float)

    def _values_from_states(self, model: Model, paths: List[str], ref: DataTable, cols):
        """values[row][frame] at the states table's rows; cols: the coordinate
        values by coordinate name."""
        pick = 0 if self.WHAT == "translation" else 1
        return [[model.frame_pose_in_ground(p, {n: v[r] for n, v in cols.items()})[pick] for p in paths]
                for r in range(len(ref.times))]

    def reference_table(self, model: Model) -> DataTable:
        """The flattened reference: <frame path>/position_x|y|z or
        <frame path>/quaternion_e0..3 per tracked frame, splined as
        GCVSplineSet(table) does (degree 5)."""
        paths = self.tracked_frame_paths()
        for p in paths:
            if model.find_frame(p) is None:
                raise ValueError(f"{type(self).__name__}: no frame '{p}' in the model")
        times, vals = self._frame_values(model, paths)
        cols = {}
        for i, p in enumerate(paths):
            flat = self._flatten(vals[:, i])
            for c, sfx in enumerate(self.SUFFIXES):
                cols[f"{p}/{sfx}"] = np.ascontiguousarray(flat[:, c])
        return DataTable(self.reference_name(), times, cols, degree=self.degree)


@dataclass
class MocoTranslationTrackingGoal(_FrameTrackingGoal):
    """MocoTranslationTrackingGoal (Moco/Moco/MocoGoal/
    MocoTranslationTrackingGoal.{h,cpp}): the integral over the phase of
    sum_f w_f |origin of model frame f in ground - reference_f(t)|^2, times the
    weight (include/mocohip.h MH_GOAL_TRANSLATION_TRACKING)."""
    name: str = "translation_tracking"
    WHAT = "translation"
    SUFFIXES = ("position_x", "position_y", "position_z")

    @staticmethod
    def _flatten(v):
        return np.asarray(v, float).reshape(len(v), 3)


@dataclass
class MocoOrientationTrackingGoal(_FrameTrackingGoal):
    """MocoOrientationTrackingGoal (Moco/Moco/MocoGoal/
    MocoOrientationTrackingGoal.{h,cpp}): the integral over the phase of
    sum_f w_f theta_f^2, theta_f the angle of the rotation between model frame
    f and the reference (rotations converted to quaternions,
    rotation_to_quaternion, splined and re-normalised), times the weight
    (include/mocohip.h MH_GOAL_ORIENTATION_TRACKING)."""
    name: str = "orientation_tracking"
    WHAT = "rotation"
    SUFFIXES = ("quaternion_e0", "quaternion_e1", "quaternion_e2", "quaternion_e3")

    @staticmethod
    def _flatten(v):
        return np.stack([rotation_to_quaternion(R) for R in np.asarray(v, float).reshape(len(v), 3, 3)])


@dataclass
class MocoAngularVelocityTrackingGoal(_FrameTrackingGoal):
    """MocoAngularVelocityTrackingGoal (Moco/Moco/MocoGoal/
    MocoAngularVelocityTrackingGoal.{h,cpp}): the integral over the phase of
    sum_f w_f |angular velocity of model frame f in ground - reference_f(t)|^2,
    times the weight (include/mocohip.h MH_GOAL_ANGULAR_VELOCITY_TRACKING).
    ``reference`` holds Vec3 columns (``values[row][frame][xyz]``, expressed in
    ground); with ``states_reference`` the angular velocities are computed at
    every row from the row's coordinate values and speeds (realizeVelocity),
    and the table needs the speed column of every coordinate that turns a
    tracked frame."""
    name: str = "angular_velocity_tracking"
    WHAT = "angular velocity"
    SUFFIXES = ("angular_velocity_x", "angular_velocity_y", "angular_velocity_z")

    @staticmethod
    def _flatten(v):
        return np.asarray(v, float).reshape(len(v), 3)

    @staticmethod
    def turning_coordinates(model: Model, paths: List[str]) -> List[str]:
        """The coordinates (by name, model order) that are the argument of a
        non-constant function on a rotation axis of a joint between ground
        and one of the frames: the speeds the frames' angular velocities
        depend on."""
        parent_joint = {j.child: j for j in model.joints}
        names = set()
        for path in paths:
            body = model.find_frame(path)[0]
            while body != "ground":
                j = parent_joint[body]
                names.update(ax.func.coord for ax in j.axes
                             if ax.type == abi.MH_AXIS_ROTATION and ax.func.kind != abi.MH_FN_CONSTANT)
                body = j.parent
        return [c.name for c in model.coordinates() if c.name in names]

    def _values_from_states(self, model: Model, paths: List[str], ref: DataTable, cols):
        bypath = {c.name: c.path + "/speed" for c in model.coordinates()}
        speeds = {}
        for name in self.turning_coordinates(model, paths):
            if bypath[name] not in ref.columns:
                raise ValueError(f"{type(self).__name__}: the states reference has no column '{bypath[name]}', "
                                 "which the angular velocity of a tracked frame depends on")
            speeds[name] = np.asarray(ref.columns[bypath[name]], float)
        vals = []
        for r in range(len(ref.times)):
            w = model._body_angular_velocities_in_ground({n: v[r] for n, v in cols.items()},
                                                         {n: v[r] for n, v in speeds.items()})
            vals.append([w[model.find_frame(p)[0]] for p in paths])
        return vals


@dataclass
class MocoAccelerationTrackingGoal(_FrameTrackingGoal):
    """MocoAccelerationTrackingGoal (Moco/Moco/MocoGoal/
    MocoAccelerationTrackingGoal.{h,cpp}): the integral over the phase of
    sum_f w_f |linear acceleration of the origin of model frame f in ground -
    reference_f(t)|^2, times the weight (include/mocohip.h
    MH_GOAL_ACCELERATION_TRACKING).  ``reference`` holds Vec3 columns
    (``values[row][frame][xyz]``, expressed in ground; the kinematic
    acceleration, without gravity).  There is no ``states_reference``: the
    reference class has no such property (states do not determine
    accelerations), and one is refused."""
    name: str = "acceleration_tracking"
    WHAT = "acceleration"
    SUFFIXES = ("acceleration_x", "acceleration_y", "acceleration_z")

    def tracked_frame_paths(self) -> List[str]:
        if self.states_reference is not None:
            raise ValueError("MocoAccelerationTrackingGoal: a states reference cannot be given (the goal has an "
                             "acceleration reference only: states do not determine accelerations)")
        return super().tracked_frame_paths()

    @staticmethod
    def _flatten(v):
        return np.asarray(v, float).reshape(len(v), 3)


@dataclass
class MocoJointReactionGoal:
    """MocoJointReactionGoal (Moco/Moco/MocoGoal/MocoJointReactionGoal.{h,cpp}):
    the integral over the phase of the weighted sum of squares of the chosen
    reaction measures of one joint, divided by the model's weight (total mass
    when there is no gravity), times the weight (include/mocohip.h
    MH_GOAL_JOINT_REACTION).  ``joint_path``: /jointset/<joint> or the joint's
    name.  ``loads_frame``: "parent" or "child", the joint frame whose body
    the load is applied to and at whose origin it is taken.
    ``expressed_in_frame_path``: the frame the load is expressed in (a body,
    ground or an offset frame; empty: the loads frame).  ``reaction_measures``:
    any of moment-x, moment-y, moment-z, force-x, force-y, force-z (empty: all
    six).  ``reaction_weights``: measure -> weight (1 unless given)."""
    name: str = "joint_reaction"
    weight: float = 1.0
    joint_path: str = ""
    loads_frame: str = "parent"
    expressed_in_frame_path: str = ""
    reaction_measures: List[str] = field(default_factory=list)
    reaction_weights: Dict[str, float] = field(default_factory=dict)

    MEASURES = ("moment-x", "moment-y", "moment-z", "force-x", "force-y", "force-z")

    def set_joint_path(self, path: str):
        self.joint_path = path

    def set_loads_frame(self, frame: str):
        self.loads_frame = frame

    def set_expressed_in_frame_path(self, path: str):
        self.expressed_in_frame_path = path

    def set_reaction_measures(self, measures: Sequence[str]):
        self.reaction_measures = list(measures)

    def set_weight(self, measure: str, weight: float):
        self.reaction_weights[measure] = float(weight)

    def measure_weights(self) -> List[float]:
        """The six weights in MEASURES order: 0 for a measure that was not
        selected; the reference's error for an unknown measure."""
        if not self.joint_path:
            raise ValueError("Expected a joint path, but property joint_path is empty.")
        if self.loads_frame not in ("parent", "child"):
            raise ValueError(f"Property 'loads_frame' (in object '{self.name}' of type MocoJointReactionGoal) "
                             f"has invalid value {self.loads_frame}; expected one of the following:  child  parent.")
        for m in self.reaction_measures:
            if m not in self.MEASURES:
                raise ValueError(f"Reaction measure '{m}' not recognized.")
        chosen = self.reaction_measures or list(self.MEASURES)
        w = [0.0] * 6
        for m in chosen:
            w[self.MEASURES.index(m)] = float(self.reaction_weights.get(m, 1.0))
        return w


def parse_muscle_output_path(model, output_path: str):
    """(muscle index, output id) of an output path ``<component>|<output>`` of
    a DeGrooteFregly2016Muscle: ``/forceset/<muscle>|<output>`` with an output
    of abi.MUSCLE_OUTPUTS (include/mocohip.h enum mh_muscle_output), or its
    path's ``/forceset/<muscle>/geometrypath|length`` / ``|lengthening_speed``.
    ValueError, naming the supported outputs, for any other component or
    output."""
    supported = ("supported: the outputs " + ", ".join(abi.MUSCLE_OUTPUTS) + " of a DeGrooteFregly2016Muscle "
                 "(<muscle path>|<output>; length and lengthening_speed also as <muscle path>/geometrypath|...)")
    comp, sep, out = output_path.partition("|")
    if not sep or not out:
        raise ValueError(f"output path '{output_path}' is not of the form <component path>|<output>; {supported}")
    path_output = comp.endswith("/geometrypath")
    if path_output:
        comp = comp[:-len("/geometrypath")]
    im = next((i for i, mu in enumerate(model.muscles) if comp in (mu.path, mu.name)), None)
    if im is None:
        raise ValueError(f"output path '{output_path}': component '{comp}' is not a DeGrooteFregly2016Muscle of "
                         f"the model; {supported}")
    if out not in abi.MUSCLE_OUTPUTS or (path_output and out not in abi.MUSCLE_OUTPUTS[:2]):
        raise ValueError(f"output path '{output_path}': no supported output '{out}'; {supported}")
    return im, abi.MUSCLE_OUTPUTS.index(out)


def parse_metabolics_output_path(model, output_path: str):
    """(component, output id, channel) of an output path ``/<component>|
    <output>`` of a Bhargava2004Metabolics component of the model
    (abi.METABOLICS_OUTPUTS, include/mocohip.h enum mh_metabolics_output; the
    list output as ``muscle_metabolic_rate:<muscle name or path>``, its channel
    the muscle's position in the component, -1 for every other output).  None
    when the path's component is no metabolics component of the model;
    ValueError for an output or a channel the component does not have."""
    comp, sep, out = output_path.partition("|")
    c = model.find_component(comp) if sep and out else None
    if c is None:
        return None
    supported = ("supported: " + ", ".join(abi.METABOLICS_OUTPUTS[:-1]) + " and " + abi.METABOLICS_OUTPUTS[-1]
                 + ":<muscle name or path>")
    name, colon, chan = out.partition(":")
    if name not in abi.METABOLICS_OUTPUTS or (name == abi.METABOLICS_OUTPUTS[-1]) != bool(colon):
        raise ValueError(f"output path '{output_path}': no supported output '{out}' of a Bhargava2004Metabolics; "
                         f"{supported}")
    if not colon:
        return c, abi.METABOLICS_OUTPUTS.index(name), -1
    for pos, mp in enumerate(c.muscles):
        mu = model.muscles[c.muscle_index(model, mp)]
        if chan in (mp.name, mp.muscle_path, mu.path, mu.name):
            return c, abi.MH_MET_COUNT - 1, pos
    raise ValueError(f"output path '{output_path}': component '{comp}' has no muscle '{chan}'")


@dataclass
class MocoOutputGoal:
    """MocoOutputGoal (Moco/Moco/MocoGoal/MocoOutputGoal.{h,cpp}): the integral
    over the phase of one scalar model output, times the weight, divided by the
    model's total mass with ``divide_by_mass`` (include/mocohip.h
    MH_GOAL_OUTPUT).  ``output_path``: an output of a DeGrooteFregly2016Muscle
    (parse_muscle_output_path), e.g. "/forceset/soleus_r|tendon_force", or of a
    Bhargava2004Metabolics component (parse_metabolics_output_path, include/
    mocohip.h MH_GOAL_METABOLICS), e.g. "/metabolics|total_metabolic_rate";
    outputs of other components are a follow-up.  ``divide_by_displacement`` needs the
    reference's calcSystemDisplacement (the displacement of the whole system's
    mass center between the initial and the final state), which is not
    available: NotImplementedError, a follow-up."""
    name: str = "output"
    weight: float = 1.0
    output_path: str = ""
    divide_by_mass: bool = False
    divide_by_displacement: bool = False

    def set_output_path(self, path: str):
        self.output_path = path

    def set_divide_by_mass(self, on: bool):
        self.divide_by_mass = bool(on)

    def set_divide_by_displacement(self, on: bool):
        self.divide_by_displacement = bool(on)


# ------------------------------------------------- functions of time ----
@dataclass
class Constant:
    """OpenSim::Constant."""
    value: float

    def ppoly(self):
        return None


@dataclass
class PiecewiseLinearFunction:
    """OpenSim::PiecewiseLinearFunction: linear between points, extended
    linearly with the end segments' slopes."""
    x: Sequence[float]
    y: Sequence[float]

    def ppoly(self):
        x, y = np.asarray(self.x, float), np.asarray(self.y, float)
        if len(x) < 2 or np.any(np.diff(x) <= 0):
            raise ValueError("PiecewiseLinearFunction needs >= 2 increasing points")
        coefs = np.zeros((len(x) - 1, 1, 2))
        coefs[:, 0, 0] = y[:-1]
        coefs[:, 0, 1] = np.diff(y) / np.diff(x)
        return x, coefs


@dataclass
class GCVSpline:
    """OpenSim::GCVSpline through (x, y) (interpolating; splines.py)."""
    degree: int
    x: Sequence[float]
    y: Sequence[float]

    def ppoly(self):
        return gcv_interpolating_ppoly(np.asarray(self.x, float), np.asarray(self.y, float),
                                       int(self.degree))


# ----------------------------------------------------- path constraints ----
@dataclass
class MocoControlBoundConstraint:
    """MocoControlBoundConstraint (Moco/Moco/MocoControlBoundConstraint.cpp):
    lower_bound(t) <= control <= upper_bound(t) for each control path, as
    path-constraint equations control - bound(t) at every mesh point."""
    name: str = "control_bound"
    control_paths: List[str] = field(default_factory=list)
    lower_bound: Optional[object] = None
    upper_bound: Optional[object] = None
    equality_with_lower: bool = False

    def add_control_path(self, path: str):
        self.control_paths.append(path)

    def set_lower_bound(self, f):
        self.lower_bound = f

    def set_upper_bound(self, f):
        self.upper_bound = f

    def set_equality_with_lower(self, v: bool):
        self.equality_with_lower = bool(v)


@dataclass
class MocoFrameDistanceConstraintPair:
    """MocoFrameDistanceConstraintPair (MocoFrameDistanceConstraint.h): the
    distance between the origins of two model frames stays within
    [minimum_distance, maximum_distance]."""
    frame1_path: str = ""
    frame2_path: str = ""
    minimum_distance: float = 0.0
    maximum_distance: float = math.inf


@dataclass
class MocoFrameDistanceConstraint:
    """MocoFrameDistanceConstraint (Moco/Moco/MocoFrameDistanceConstraint.
    {h,cpp}): per frame pair one path-constraint equation, the squared
    distance between the two frame origins in ground -- or of its projection
    onto ``projection_vector`` ("vector") or onto the plane normal to it
    ("plane") -- bounded by [minimum^2, maximum^2] at every mesh point."""
    name: str = "frame_distance"
    frame_pairs: List[MocoFrameDistanceConstraintPair] = field(default_factory=list)
    projection: str = "none"
    projection_vector: Optional[Sequence[float]] = None

    def add_frame_pair(self, pair, frame2_path=None, minimum_distance=0.0, maximum_distance=math.inf):
        if not isinstance(pair, MocoFrameDistanceConstraintPair):
            pair = MocoFrameDistanceConstraintPair(pair, frame2_path, minimum_distance, maximum_distance)
        self.frame_pairs.append(pair)
        return pair

    def set_projection(self, projection: str):
        self.projection = projection

    def set_projection_vector(self, v):
        self.projection_vector = tuple(float(a) for a in v)


@dataclass
class ImplicitAuxiliaryDerivativesTerm:
    """MocoDirectCollocationSolver minimize_implicit_auxiliary_derivatives /
    implicit_auxiliary_derivatives_weight as an objective term
    (CasOCTranscription.cpp:534-545): weight * integral of the sum of squared
    implicit auxiliary derivatives."""
    name: str = "auxiliary_derivatives"
    weight: float = 1.0


@dataclass
class MocoParameter:
    """MocoParameter (Moco/Moco/MocoParameter.h:91-170): an NLP variable
    written into the property ``property_name`` of every component in
    ``component_paths`` before each evaluation; ``property_element`` picks
    the element of a vector property (mass_center: 0-2, inertia: 0-5 = xx yy
    zz xy xz yz), -1 for a scalar one.  Components are named by name or path
    (a Body, SpringGeneralizedForce, CoordinateActuator or DGF muscle);
    supported properties: Body mass / mass_center / inertia,
    SpringGeneralizedForce stiffness / rest_length / viscosity,
    CoordinateActuator optimal_force, muscle max_isometric_force
    (include/mocohip.h mh_parameter_kind)."""
    name: str
    component_paths: Sequence[str]
    property_name: str
    bounds: MocoBounds = field(default_factory=MocoBounds)
    property_element: int = -1


class MocoProblem:
    """Single-phase MocoProblem (MocoProblem.h)."""

    def __init__(self, model: Optional[Model] = None):
        self.model = model
        self.time_initial = MocoBounds()
        self.time_final = MocoBounds()
        self.state_infos: Dict[str, MocoVariableInfo] = {}
        self.control_infos: Dict[str, MocoVariableInfo] = {}
        self.goals: List[object] = []
        self.path_constraints: List[object] = []
        self.position_motion: Optional[DataTable] = None
        self.default_speed_bounds = MocoBounds(-50.0, 50.0)
        self.bound_activation_from_excitation = True
        # MocoPhase kinematic_constraint_bounds / multiplier_bounds
        # (MocoProblem.cpp:42-43)
        self.kinematic_constraint_bounds = MocoBounds(0.0, 0.0)
        self.multiplier_bounds = MocoBounds(-1000.0, 1000.0)
        self.parameters: List[MocoParameter] = []

    def set_model(self, model: Model):
        self.model = model

    def set_kinematic_constraint_bounds(self, bounds):
        self.kinematic_constraint_bounds = MocoBounds.of(bounds)

    def set_multiplier_bounds(self, bounds):
        self.multiplier_bounds = MocoBounds.of(bounds)

    def set_time_bounds(self, initial, final):
        self.time_initial = MocoBounds.of(initial)
        self.time_final = MocoBounds.of(final)

    def set_state_info(self, name, bounds=None, initial=None, final=None):
        self.state_infos[name] = MocoVariableInfo(
            MocoBounds.of(bounds), MocoBounds.of(initial), MocoBounds.of(final))

    def set_control_info(self, name, bounds=None, initial=None, final=None):
        self.control_infos[name] = MocoVariableInfo(
            MocoBounds.of(bounds), MocoBounds.of(initial), MocoBounds.of(final))

    def add_parameter(self, name: str, component_paths, property_name: str, bounds=None,
                      property_element: int = -1) -> MocoParameter:
        """MocoProblem::addParameter (MocoProblem.h: the MocoParameter
        constructors, MocoParameter.h:100-112)."""
        paths = [component_paths] if isinstance(component_paths, str) else list(component_paths)
        par = MocoParameter(name, paths, property_name, MocoBounds.of(bounds), int(property_element))
        self.parameters.append(par)
        return par

    def add_goal(self, goal):
        self.goals.append(goal)
        return goal

    def set_position_motion(self, kinematics: DataTable):
        """PositionMotion::createFromTable (Components/PositionMotion.cpp:
        121-155): every coordinate prescribed by a GCVSpline (degree 5 unless
        the table says otherwise) of the column named by its value path
        ("/jointset/<joint>/<coordinate>/value")."""
        self.position_motion = kinematics

    def add_path_constraint(self, constraint):
        self.path_constraints.append(constraint)
        return constraint

    def create_rep(self) -> "ProblemRep":
        return ProblemRep(self)


def _vi(info: MocoVariableInfo) -> abi.mh_variable_info:
    v = abi.mh_variable_info()
    for dst, src in ((v.bounds, info.bounds), (v.initial, info.initial),
                     (v.final, info.final)):
        dst.lower, dst.upper = src.lower, src.upper
    return v


class ProblemRep:
    """MocoProblemRep: resolves default bounds and lowers to mh_problem."""

    def __init__(self, problem: MocoProblem):
        self.problem = problem
        model = problem.model
        path_eqs, bound_tables, frame_terms = self._path_equations(problem)
        kin = problem.position_motion
        extra = list(bound_tables)
        if kin is not None:
            qpaths = [c.path + "/value" for c in model.coordinates()]
            missing = [q for q in qpaths if q not in kin.columns]
            if missing:
                raise ValueError(f"PositionMotion: no kinematics for {missing}")
            extra.append(DataTable("__position_motion", np.asarray(kin.times, float),
                                   {q: np.asarray(kin.columns[q], float) for q in qpaths},
                                   degree=kin.degree))
        self.compiled: CompiledModel = model.compile(extra_tables=extra)
        # prescribed kinematics: coordinate values and speeds are not states
        # (MocoProblemRep.cpp:541-555)
        self.prescribed_kinematics = kin is not None
        self.state_names = [n for n in self.compiled.state_names
                            if not (self.prescribed_kinematics and
                                    (n.endswith("/value") or n.endswith("/speed")))]
        self.control_names = self.compiled.control_names
        sinfo: Dict[str, MocoVariableInfo] = {}
        cinfo: Dict[str, MocoVariableInfo] = {}
        for k, v in problem.state_infos.items():
            sinfo[k] = MocoVariableInfo(v.bounds, v.initial, v.final)
        for k, v in problem.control_infos.items():
            cinfo[k] = MocoVariableInfo(v.bounds, v.initial, v.final)
        # statebounds_ outputs: DGF normalized tendon force in [0, 5]
        # (DeGrooteFregly2016Muscle.h:131-132,304-305).
        for m in model.muscles:
            if not m.ignore_tendon_compliance:
                nm = m.path + "/normalized_tendon_force"
                info = sinfo.setdefault(nm, MocoVariableInfo())
                if not info.bounds.is_set():
                    info.bounds = MocoBounds(0.0, 5.0)
        # coordinates: range; speeds: default speed bounds (:336-362)
        for c in model.coordinates():
            vn, sn = c.path + "/value", c.path + "/speed"
            info = sinfo.setdefault(vn, MocoVariableInfo())
            if not info.bounds.is_set():
                info.bounds = MocoBounds(float(c.range[0]), float(c.range[1]))
            info = sinfo.setdefault(sn, MocoVariableInfo())
            if not info.bounds.is_set():
                info.bounds = problem.default_speed_bounds
        # controls from actuator min/max; activation from excitation (:394-427)
        for a in model.actuators:
            info = cinfo.setdefault(a.path, MocoVariableInfo())
            if not info.bounds.is_set():
                info.bounds = MocoBounds(float(a.min_control), float(a.max_control))
            if (problem.bound_activation_from_excitation and
                    isinstance(a, DeGrooteFregly2016Muscle) and
                    not a.ignore_activation_dynamics):
                an = a.path + "/activation"
                ai = sinfo.setdefault(an, MocoVariableInfo())
                if not ai.bounds.is_set():
                    ai.bounds = info.bounds
        self.state_infos = [sinfo.get(n, MocoVariableInfo()) for n in self.state_names]
        self.control_infos = [cinfo.get(n, MocoVariableInfo()) for n in self.control_names]

        # goals (endpoint-constraint mode goals become endpoint equations,
        # in goal order: MocoProblemRep::createEndpointConstraintNames)
        goals, gidx, gcol, gw = [], [], [], []
        goal_names: List[str] = []   # the mh_goal entries' goal names (objective breakdown)
        endpoint: List[abi.mh_endpoint_equation] = []
        sidx = {n: i for i, n in enumerate(self.state_names)}
        cidx = {n: i for i, n in enumerate(self.control_names)}
        self.extra_tables: List[DataTable] = []
        for g in problem.goals:
            if isinstance(g, MocoInitialActivationGoal):
                if g.mode != "endpoint_constraint":
                    raise NotImplementedError("MocoInitialActivationGoal in cost mode "
                                              "(only the endpoint-constraint default is on the "
                                              "hot path)")
                for mu in model.muscles:
                    if mu.ignore_activation_dynamics:
                        continue
                    e = abi.mh_endpoint_equation()
                    e.kind = abi.MH_ENDPOINT_INITIAL_ACTIVATION
                    e.index_a = cidx[mu.path]
                    e.index_b = sidx[mu.path + "/activation"]
                    e.g.lower, e.g.upper = 0.0, 0.0
                    endpoint.append(e)
                continue
            gs = abi.mh_goal()
            gs.weight = float(g.weight)
            gs.term_begin = len(gidx)
            gs.table = -1
            gs.exponent = 2
            if isinstance(g, MocoControlGoal):
                gs.kind = abi.MH_GOAL_CONTROL
                gs.exponent = int(g.exponent)
                if gs.exponent < 2:
                    raise ValueError("Exponent must be 2 or greater.")
                for n in g.control_weights:   # MocoControlGoal.cpp:64-71
                    if n not in cidx:
                        raise ValueError(f"Unrecognized control '{n}'.")
                for n in self.control_names:
                    w = float(g.control_weights.get(n, 1.0))
                    if w != 0.0:
                        gidx.append(cidx[n]); gcol.append(-1); gw.append(w)
            elif isinstance(g, MocoStateTrackingGoal):
                gs.kind = abi.MH_GOAL_STATE_TRACKING
                for n in g.state_weights:   # MocoStateTrackingGoal.cpp:45-52
                    if n not in sidx:
                        raise ValueError(f"Weight provided with name '{n}' but this is not a "
                                         "recognized state.")
                ref = g.reference
                if ref.name not in self.compiled.table_index:
                    raise ValueError(f"reference table {ref.name} not in model")
                gs.table = self.compiled.table_index[ref.name]
                cols = self.compiled.table_columns[ref.name]
                for ci, n in enumerate(cols):
                    if n not in sidx:
                        raise ValueError(f"State reference '{n}' unrecognized.")
                    gidx.append(sidx[n]); gcol.append(ci)
                    gw.append(float(g.state_weights.get(n, 1.0)))
            elif isinstance(g, MocoFinalTimeGoal):
                gs.kind = abi.MH_GOAL_FINAL_TIME
            elif isinstance(g, MocoMarkerFinalGoal):
                if kin is not None:
                    raise NotImplementedError("MocoMarkerFinalGoal with prescribed kinematics "
                                              "(the final coordinates are not NLP states)")
                mk = model.markers.get(g.point_name)
                if mk is None:
                    raise ValueError(f"MocoMarkerFinalGoal: no point '{g.point_name}' in the model")
                body = self.compiled.body_index[mk.body]
                gs.kind = abi.MH_GOAL_MARKER_FINAL
                ref = [float(v) for v in g.reference_location]
                for ci, v in enumerate([float(v) for v in mk.location] + ref):
                    gidx.append(body); gcol.append(ci); gw.append(v)
            elif isinstance(g, MocoMarkerTrackingGoal):
                if kin is not None:
                    raise NotImplementedError("MocoMarkerTrackingGoal with prescribed kinematics "
                                              "(the coordinates are not NLP states)")
                gs.kind = abi.MH_GOAL_MARKER_TRACKING
                self._marker_tracking_terms(model, g, gs, gidx, gcol, gw)
            elif isinstance(g, (MocoTranslationTrackingGoal, MocoOrientationTrackingGoal,
                                MocoAngularVelocityTrackingGoal)):
                if kin is not None:
                    raise NotImplementedError(f"{type(g).__name__} with prescribed kinematics "
                                              "(the coordinates are not NLP states)")
                self._frame_tracking_terms(model, g, gs, gidx, gcol, gw)
            elif isinstance(g, MocoAccelerationTrackingGoal):
                if kin is not None:
                    raise NotImplementedError("MocoAccelerationTrackingGoal with prescribed kinematics "
                                              "(the accelerations are not the NLP's)")
                if problem.parameters:
                    raise NotImplementedError("MocoAccelerationTrackingGoal with MocoParameters "
                                              "(the goals' gradient along a parameter is defined as 0)")
                self._frame_tracking_terms(model, g, gs, gidx, gcol, gw)
            elif isinstance(g, MocoJointReactionGoal):
                if kin is not None:
                    raise NotImplementedError("MocoJointReactionGoal with prescribed kinematics "
                                              "(the accelerations are not the NLP's)")
                if problem.parameters:
                    raise NotImplementedError("MocoJointReactionGoal with MocoParameters "
                                              "(the load reads the mass properties)")
                self._joint_reaction_terms(model, g, gs, gidx, gcol, gw)
            elif isinstance(g, MocoOutputGoal):
                # MocoOutputGoal::initializeOnModelImpl's check, then one term:
                # the muscle, the output, the divisor (Model::getTotalMass)
                if not g.output_path:
                    raise ValueError("No output_path provided.")
                if g.divide_by_displacement:
                    raise NotImplementedError("MocoOutputGoal with divide_by_displacement "
                                              "(calcSystemDisplacement is not available)")
                if problem.parameters:
                    raise NotImplementedError("MocoOutputGoal with MocoParameters "
                                              "(the goals' gradient along a parameter is defined as 0)")
                den = 1.0
                if g.divide_by_mass:
                    den = 0.0
                    for body in model.bodies.values():
                        den += float(body.mass)
                met = parse_metabolics_output_path(model, g.output_path)
                if met is not None:
                    # an output of a Bhargava2004Metabolics: the component
                    # travels in the goal's terms (MH_GOAL_METABOLICS)
                    gs.kind = abi.MH_GOAL_METABOLICS
                    bi, bc, bw = met[0].term_block(model, met[1], met[2], den)
                    gidx.extend(bi); gcol.extend(bc); gw.extend(bw)
                else:
                    im, which = parse_muscle_output_path(model, g.output_path)
                    gs.kind = abi.MH_GOAL_OUTPUT
                    gidx.append(im); gcol.append(which); gw.append(den)
            elif isinstance(g, ImplicitAuxiliaryDerivativesTerm):
                gs.kind = abi.MH_GOAL_AUX_DERIVATIVES
                naux = sum(1 for m in model.muscles if not m.ignore_tendon_compliance
                           and m.tendon_compliance_dynamics_mode == "implicit")
                for k in range(naux):
                    gidx.append(k); gcol.append(-1); gw.append(1.0)
            elif isinstance(g, MocoSumSquaredStateGoal):
                gs.kind = abi.MH_GOAL_SUM_SQUARED_STATE
                for n in g.state_weights:   # MocoSumSquaredStateGoal.cpp:37-45
                    if n not in sidx:
                        raise ValueError(f"Weight provided with name '{n}' but this is not a "
                                         "recognized state.")
                for n in self.state_names:
                    w = float(g.state_weights.get(n, 1.0))
                    if w != 0.0:
                        gidx.append(sidx[n]); gcol.append(-1); gw.append(w)
            else:
                raise TypeError(f"unsupported goal {type(g).__name__}")
            gs.term_count = len(gidx) - gs.term_begin
            goals.append(gs)
            goal_names.append(getattr(g, "name", "") or type(g).__name__)

        # frame-distance equations: the bodies, and nine terms that belong to
        # no goal (include/mocohip.h mh_path_kind)
        for e, (b1, b2, vals) in zip([q for q in path_eqs if q.kind != abi.MH_PATH_CONTROL_BOUND],
                                     frame_terms):
            if kin is not None:
                raise NotImplementedError("MocoFrameDistanceConstraint with prescribed kinematics "
                                          "(the coordinates are not NLP states)")
            e.index, e.table = self.compiled.body_index[b1], self.compiled.body_index[b2]
            e.column = len(gidx)
            for v in vals:
                gidx.append(0); gcol.append(0); gw.append(float(v))

        self._sinfo = (abi.mh_variable_info * max(1, len(self.state_infos)))(
            *[_vi(i) for i in self.state_infos])
        self._cinfo = (abi.mh_variable_info * max(1, len(self.control_infos)))(
            *[_vi(i) for i in self.control_infos])
        self._goals = (abi.mh_goal * max(1, len(goals)))(*goals)
        self.goal_names = goal_names
        self._gidx = np.ascontiguousarray(gidx + [0], np.int32)
        self._gcol = np.ascontiguousarray(gcol + [0], np.int32)
        self._gw = np.ascontiguousarray(gw + [0.0], float)
        p = abi.mh_problem()
        p.model = self.compiled.struct
        p.time_initial.lower, p.time_initial.upper = problem.time_initial.lower, problem.time_initial.upper
        p.time_final.lower, p.time_final.upper = problem.time_final.lower, problem.time_final.upper
        p.state_infos = self._sinfo
        p.control_infos = self._cinfo
        p.ngoals = len(goals)
        p.nterms = len(gidx)
        p.goals = self._goals
        p.goal_index = abi.iptr(self._gidx)
        p.goal_column = abi.iptr(self._gcol)
        p.goal_weight = abi.dptr(self._gw)
        for e in path_eqs:
            if e.kind == abi.MH_PATH_CONTROL_BOUND and e.table >= 0:   # bound table index: after the model's own
                e.table = self.compiled.table_index[bound_tables[e.table].name]
        self._path = (abi.mh_path_equation * max(1, len(path_eqs)))(*path_eqs)
        p.prescribed_kinematics = 0
        if kin is not None:
            p.prescribed_kinematics = 1
            p.kinematics_table = self.compiled.table_index["__position_motion"]
            self._kin_cols = np.arange(self.compiled.nq, dtype=np.int32)
            p.kinematics_column = abi.iptr(self._kin_cols)
        p.npath = len(path_eqs)
        p.path = self._path
        self._endpoint = (abi.mh_endpoint_equation * max(1, len(endpoint)))(*endpoint)
        p.nendpoint = len(endpoint)
        p.endpoint = self._endpoint
        p.multiplier_bounds.lower = problem.multiplier_bounds.lower
        p.multiplier_bounds.upper = problem.multiplier_bounds.upper
        p.kinematic_constraint_bounds.lower = problem.kinematic_constraint_bounds.lower
        p.kinematic_constraint_bounds.upper = problem.kinematic_constraint_bounds.upper
        # MocoParameters: bounds per parameter, one target per written property
        targets, pbounds = self._parameter_targets(problem, self.compiled)
        self.parameter_names = [par.name for par in problem.parameters]
        self._pbounds = (abi.mh_bounds * max(1, len(pbounds)))(*pbounds)
        self._ptargets = (abi.mh_parameter_target * max(1, len(targets)))(*targets)
        p.nparameters = len(pbounds)
        p.nparameter_targets = len(targets)
        p.parameter_bounds = self._pbounds
        p.parameter_targets = self._ptargets
        self.num_kinematic_constraints = len(model.constraints)
        self.num_endpoint_equations = len(endpoint)
        self.num_path_equations = len(path_eqs)
        self.struct = p
        self.num_states = len(self.state_names)
        self.num_controls = len(self.control_names)
        self.nq = self.compiled.nq
        # implicit auxiliary dynamics: DGF muscles with compliant tendons in
        # tendon_compliance_dynamics_mode "implicit" (one derivative variable
        # and one residual row per grid point each)
        self.num_aux_residuals = sum(
            1 for m in model.muscles
            if not m.ignore_tendon_compliance and m.tendon_compliance_dynamics_mode == "implicit")
        # the reference's names of the other variable blocks (MocoTrajectory
        # columns).  Multipliers: MocoProblemRep.cpp:202-230 names them
        # lambda_cid<c>_p<i> after the Simbody ConstraintIndex c, and OpenSim
        # gives every Coordinate a (disabled) lock constraint of its own
        # before the model's ConstraintSet, so the enabled couplers are
        # ConstraintIndex ncoord, ncoord + 1, ... (Rajagopal 18: 21 coordinates
        # -> lambda_cid21_p0, lambda_cid22_p0 in std_testMocoInverse_subject_
        # 18musc_solution.sto).  Slacks: the same with gamma
        # (MocoCasOCProblem.cpp:186-201).  Implicit auxiliary derivatives:
        # <component>/implicitderiv_<state> (MocoProblemRep.cpp:445-460,
        # MocoCasOCProblem.cpp:92-97), after the accelerations <coordinate>/accel
        # of implicit multibody dynamics (CasOCProblem.h:363-377).
        ncoord = len(model.coordinates())
        self.multiplier_names = [f"lambda_cid{ncoord + i}_p0" for i in range(len(model.constraints))]
        self.slack_names_all = [f"gamma_cid{ncoord + i}_p0" for i in range(len(model.constraints))]
        self.aux_derivative_names = [
            m.path + "/implicitderiv_normalized_tendon_force" for m in model.muscles
            if not m.ignore_tendon_compliance and m.tendon_compliance_dynamics_mode == "implicit"]
        self.accel_names_all = [n[:-len("speed")] + "accel" for n in self.state_names if n.endswith("/speed")]

    @staticmethod
    def _parameter_targets(problem: MocoProblem, compiled: CompiledModel):
        """MocoParameter::initializeOnModel (MocoParameter.cpp): each
        component path must name a component with the property; vector
        properties need an element in range, scalar ones none."""
        model = problem.model
        scalar = {"mass": abi.MH_PARAM_BODY_MASS, "stiffness": abi.MH_PARAM_SPRING_STIFFNESS,
                  "rest_length": abi.MH_PARAM_SPRING_REST_LENGTH, "viscosity": abi.MH_PARAM_SPRING_VISCOSITY,
                  "optimal_force": abi.MH_PARAM_ACTUATOR_OPTIMAL_FORCE,
                  "max_isometric_force": abi.MH_PARAM_MUSCLE_MAX_ISOMETRIC_FORCE}
        vector = {"mass_center": (abi.MH_PARAM_BODY_MASS_CENTER, 3), "inertia": (abi.MH_PARAM_BODY_INERTIA, 6)}

        def find(path):
            key = path.rstrip("/").split("/")[-1]
            for b in model.bodies.values():
                if path in (b.name, "/bodyset/" + b.name, "/" + b.name):
                    return "body", compiled.body_index[b.name]
            for i, f in enumerate(model.springs):
                if path in (f.name, f.path) or key == f.name:
                    return "spring", i
            for i, a in enumerate(model.actuators):
                if path in (a.name, a.path):
                    return ("muscle", model.muscles.index(a)) if isinstance(a, DeGrooteFregly2016Muscle) \
                        else ("actuator", i)
            raise ValueError(f"MocoParameter: no component '{path}' in the model")
        owner = {abi.MH_PARAM_BODY_MASS: "body", abi.MH_PARAM_BODY_MASS_CENTER: "body",
                 abi.MH_PARAM_BODY_INERTIA: "body", abi.MH_PARAM_SPRING_STIFFNESS: "spring",
                 abi.MH_PARAM_SPRING_REST_LENGTH: "spring", abi.MH_PARAM_SPRING_VISCOSITY: "spring",
                 abi.MH_PARAM_ACTUATOR_OPTIMAL_FORCE: "actuator",
                 abi.MH_PARAM_MUSCLE_MAX_ISOMETRIC_FORCE: "muscle"}
        targets, bounds = [], []
        names = set()
        for ip, par in enumerate(problem.parameters):
            if par.name in names:
                raise ValueError(f"MocoParameter '{par.name}': duplicate name")
            names.add(par.name)
            if not par.component_paths:
                raise ValueError(f"MocoParameter '{par.name}': no component paths")
            if par.property_name in vector:
                kind, nel = vector[par.property_name]
                if not 0 <= par.property_element < nel:
                    raise ValueError(f"MocoParameter '{par.name}': property '{par.property_name}' needs an "
                                     f"element in [0, {nel})")
                elem = par.property_element
            elif par.property_name in scalar:
                if par.property_element >= 0:
                    raise ValueError(f"MocoParameter '{par.name}': a property element was given for the "
                                     f"scalar property '{par.property_name}'")
                kind, elem = scalar[par.property_name], 0
            else:
                raise NotImplementedError(f"MocoParameter '{par.name}': property '{par.property_name}' is "
                                          "not a parameterizable property of this build")
            for path in par.component_paths:
                what, idx = find(path)
                if what != owner[kind]:
                    raise ValueError(f"MocoParameter '{par.name}': component '{path}' ({what}) has no "
                                     f"property '{par.property_name}'")
                t = abi.mh_parameter_target()
                t.parameter, t.kind, t.index, t.element = ip, kind, idx, elem
                targets.append(t)
            b = abi.mh_bounds()
            b.lower, b.upper = par.bounds.lower, par.bounds.upper
            bounds.append(b)
        return targets, bounds

    @staticmethod
    def _path_equations(problem: MocoProblem):
        """Expand path constraints to mh_path_equation rows, with the
        initializeOnModel checks of MocoControlBoundConstraint.cpp:38-118.
        Bound functions other than Constant become piecewise polynomial
        tables appended to the model's (indices into the returned list)."""
        names = problem.model.control_names()
        cidx = {n: i for i, n in enumerate(names)}
        eqs: List[abi.mh_path_equation] = []
        tables: List[DataTable] = []
        frame_terms: List[tuple] = []   # per frame-distance equation: body 1, body 2, nine doubles
        for ci, pc in enumerate(problem.path_constraints):
            if isinstance(pc, MocoFrameDistanceConstraint):
                ProblemRep._frame_distance_equations(problem.model, pc, eqs, frame_terms)
                continue
            if not isinstance(pc, MocoControlBoundConstraint):
                raise TypeError(f"unsupported path constraint {type(pc).__name__}")
            has_lo, has_up = pc.lower_bound is not None, pc.upper_bound is not None
            if pc.control_paths and not (has_lo or has_up):
                continue   # the reference warns and adds no equations
            for path in pc.control_paths:
                if path not in cidx:
                    raise ValueError(f"Control path '{path}' was provided but no such "
                                     "control exists in the model.")
            if pc.equality_with_lower and has_up:
                raise ValueError("If equality_with_lower==true, upper bound function "
                                 "must not be set.")
            if pc.equality_with_lower and not has_lo:
                raise ValueError("If equality_with_lower==true, lower bound function "
                                 "must be set.")
            for f in (pc.lower_bound, pc.upper_bound):
                if isinstance(f, GCVSpline):
                    lo, hi = min(f.x), max(f.x)
                    if lo > problem.time_initial.lower:
                        raise ValueError(f"The function's minimum domain value ({lo}) must be "
                                         "less than or equal to the minimum possible initial "
                                         f"time ({problem.time_initial.lower}).")
                    if hi < problem.time_final.upper:
                        raise ValueError(f"The function's maximum domain value ({hi}) must be "
                                         "greater than or equal to the maximum possible final "
                                         f"time ({problem.time_final.upper}).")

            def bound_ref(f, which):
                pp = f.ppoly()
                if pp is None:
                    return -1, 0, float(f.value)
                name = f"__path{ci}_{which}"
                if not any(t.name == name for t in tables):
                    br, cf = pp
                    tables.append(DataTable(name=name, times=np.asarray(br, float),
                                            columns={"bound": np.zeros(len(br))},
                                            ppoly=(np.asarray(br, float), np.asarray(cf, float))))
                return [t.name for t in tables].index(name), 0, 0.0

            for path in pc.control_paths:
                for which, f in (("lower", pc.lower_bound), ("upper", pc.upper_bound)):
                    if f is None:
                        continue
                    e = abi.mh_path_equation()
                    e.kind = abi.MH_PATH_CONTROL_BOUND
                    e.index = cidx[path]
                    e.table, e.column, e.value = bound_ref(f, which)
                    if pc.equality_with_lower:
                        e.g.lower, e.g.upper = 0.0, 0.0
                    elif which == "lower":
                        e.g.lower, e.g.upper = 0.0, math.inf
                    else:
                        e.g.lower, e.g.upper = -math.inf, 0.0
                    eqs.append(e)
        return eqs, tables, frame_terms

    def _marker_tracking_terms(self, model: Model, g: "MocoMarkerTrackingGoal", gs, gidx, gcol, gw):
        """MocoMarkerTrackingGoal::initializeOnModelImpl
        (MocoMarkerTrackingGoal.cpp:28-83): its checks and messages; four
        terms per tracked marker (include/mocohip.h MH_GOAL_MARKER_TRACKING),
        the weights matched by reference index."""
        ref = g.markers_reference
        if ref is None:
            raise ValueError("MocoMarkerTrackingGoal: no markers reference")
        check_redundant_labels(ref.labels)
        if ref.name not in self.compiled.table_index:
            raise ValueError(f"reference table {ref.name} not in model")
        gs.table = self.compiled.table_index[ref.name]
        cols = self.compiled.table_columns[ref.name]
        by_name: Dict[str, object] = {}
        for mk in model.markers.values():
            by_name.setdefault(mk.name, mk)    # the first of that name, as the C++ builder
        weights = ref.weights()
        for i, label in enumerate(ref.labels):
            mk = model.markers.get(label)      # a component path ...
            if mk is None:
                mk = by_name.get(label)        # ... or a name in the marker set
            if mk is None:
                if not g.allow_unused_references:
                    raise ValueError(f"Marker '{label}' unrecognized by the specified model.")
                continue
            if weights[i] < 0:
                raise ValueError(f"MocoMarkerTrackingGoal: negative weight {weights[i]} of marker '{label}'")
            body = self.compiled.body_index[mk.body]
            for c in range(3):
                col = f"{label}_{c + 1}"
                if col not in cols:
                    raise ValueError(f"reference table {ref.name} has no column '{col}'")
                gidx.append(body); gcol.append(cols.index(col)); gw.append(float(mk.location[c]))
            gidx.append(body); gcol.append(-1); gw.append(weights[i])

    def _frame_tracking_terms(self, model: Model, g: "_FrameTrackingGoal", gs, gidx, gcol, gw):
        """MocoTranslationTrackingGoal / MocoOrientationTrackingGoal::
        initializeOnModelImpl: four terms per tracked frame (kind 9, as a
        marker's; kind 15 the same with the acceleration columns; kind 12:
        the angular-velocity columns with zero weights, then the weight) or
        ten (kind 10: R_BO, the quaternion columns, the
        weight);
        include/mocohip.h."""
        orient = isinstance(g, MocoOrientationTrackingGoal)
        angvel = isinstance(g, MocoAngularVelocityTrackingGoal)
        gs.kind = (abi.MH_GOAL_ORIENTATION_TRACKING if orient else
                   abi.MH_GOAL_ANGULAR_VELOCITY_TRACKING if angvel else
                   abi.MH_GOAL_ACCELERATION_TRACKING if isinstance(g, MocoAccelerationTrackingGoal) else
                   abi.MH_GOAL_TRANSLATION_TRACKING)
        paths = g.tracked_frame_paths()
        name = g.reference_name()
        if name not in self.compiled.table_index:
            raise ValueError(f"reference table {name} not in model")
        gs.table = self.compiled.table_index[name]
        cols = self.compiled.table_columns[name]
        for path in paths:
            fr = model.find_frame(path)
            if fr is None:
                raise ValueError(f"{type(g).__name__}: no frame '{path}' in the model")
            w = g.weight_for_frame(path)
            if w < 0:
                raise ValueError(f"{type(g).__name__}: negative weight {w} of frame '{path}'")
            body = -1 if fr[0] == "ground" else self.compiled.body_index[fr[0]]
            ci = []
            for sfx in g.SUFFIXES:
                col = f"{path}/{sfx}"
                if col not in cols:
                    raise ValueError(f"reference table {name} has no column '{col}'")
                ci.append(cols.index(col))
            if orient:
                R = model.find_frame_orientation(path)
                for k in range(9):
                    gidx.append(body); gcol.append(ci[k] if k < 4 else -1); gw.append(float(R[k // 3, k % 3]))
            else:
                for c in range(3):   # angular velocity: the frame's location is not used
                    gidx.append(body); gcol.append(ci[c]); gw.append(0.0 if angvel else float(fr[1][c]))
            gidx.append(body); gcol.append(-1); gw.append(w)

    def _joint_reaction_terms(self, model: Model, g: "MocoJointReactionGoal", gs, gidx, gcol, gw):
        """MocoJointReactionGoal::initializeOnModelImpl: sixteen terms
        (include/mocohip.h MH_GOAL_JOINT_REACTION) -- R_EO with the
        expressed-in body, the six measure weights, the loads frame with the
        denominator."""
        gs.kind = abi.MH_GOAL_JOINT_REACTION
        w6 = g.measure_weights()   # (the reference checks the joint path and the loads frame first)
        joint = next((j for j in model.joints if g.joint_path in (j.name, "/jointset/" + j.name)), None)
        if joint is None:
            raise ValueError(f"MocoJointReactionGoal: no joint '{g.joint_path}' in the model")
        for m, w in zip(g.MEASURES, w6):
            if w < 0:
                raise ValueError(f"MocoJointReactionGoal: negative weight {w} of measure '{m}'")
        child = g.loads_frame == "child"
        b = self.compiled.body_index[joint.child]
        if g.expressed_in_frame_path:
            fr = model.find_frame(g.expressed_in_frame_path)
            if fr is None:
                raise ValueError(f"MocoJointReactionGoal: no frame '{g.expressed_in_frame_path}' in the model")
            e, R = self.compiled.body_index[fr[0]], model.find_frame_orientation(g.expressed_in_frame_path)
        else:   # the joint's own frame on that side
            e = self.compiled.body_index[joint.child if child else joint.parent]
            R = body_fixed_xyz(joint.orient_in_child if child else joint.orient_in_parent)
        # Model::getTotalMass x |gravity| (the total mass without gravity)
        den = 0.0
        for body in model.bodies.values():
            den += float(body.mass)
        g0, g1, g2 = (float(v) for v in model.gravity)
        gmag = math.sqrt((g0 * g0 + g1 * g1) + g2 * g2)
        if gmag > float(np.finfo(float).eps) ** 0.875:   # SimTK::SignificantReal
            den *= gmag
        for k in range(9):
            gidx.append(b); gcol.append(e); gw.append(float(R[k // 3, k % 3]))
        for w in w6:
            gidx.append(b); gcol.append(-1); gw.append(w)
        gidx.append(b); gcol.append(1 if child else 0); gw.append(den)

    @staticmethod
    def _frame_distance_equations(model: Model, pc: "MocoFrameDistanceConstraint", eqs, frame_terms):
        """MocoFrameDistanceConstraint::initializeOnModelImpl
        (MocoFrameDistanceConstraint.cpp:56-112): its checks and messages,
        bounds [minimum^2, maximum^2], one equation per pair."""
        pairs = []
        for pair in pc.frame_pairs:
            frames = []
            for path in (pair.frame1_path, pair.frame2_path):
                fr = model.find_frame(path)
                if fr is None:
                    raise ValueError(f"Could not find frame '{path}'.")
                frames.append(fr)
            lo, hi = float(pair.minimum_distance), float(pair.maximum_distance)
            if lo < 0:
                raise ValueError("Expected the minimum distance for this frame pair to "
                                 f"non-negative, but it is {lo}.")
            if hi < 0:
                raise ValueError("Expected the maximum distance for this frame pair "
                                 f"to non-negative, but it is {hi}.")
            if lo > hi:
                raise ValueError("Expected the minimum distance for this frame pair "
                                 "to be less than or equal to the maximum distance, "
                                 f"but they are {lo} and {hi}, respectively.")
            pairs.append((frames, lo, hi))
        kinds = {"none": abi.MH_PATH_FRAME_DISTANCE, "vector": abi.MH_PATH_FRAME_DISTANCE_VECTOR,
                 "plane": abi.MH_PATH_FRAME_DISTANCE_PLANE}
        if pc.projection not in kinds:
            raise ValueError("Expected 'projection' to be 'none', 'vector', or 'plane', but "
                             f"got '{pc.projection}'.")
        n = [0.0, 0.0, 0.0]
        if pc.projection != "none":
            if pc.projection_vector is None or len(pc.projection_vector) == 0:
                raise ValueError("Must provide a value for 'projection_vector'.")
            if not any(float(v) != 0.0 for v in pc.projection_vector):
                raise ValueError("'projection_vector' must not be the zero vector.")
            n = unit3(pc.projection_vector)   # SimTK::UnitVec3
        for (f1, f2), lo, hi in pairs:
            e = abi.mh_path_equation()
            e.kind = kinds[pc.projection]
            e.index = e.table = -1   # the bodies and the term offset: ProblemRep.__init__
            e.g.lower, e.g.upper = lo * lo, hi * hi
            eqs.append(e)
            frame_terms.append((f1[0], f2[0], list(f1[1]) + list(f2[1]) + n))
