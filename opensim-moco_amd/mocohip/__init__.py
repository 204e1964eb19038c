"""mocohip — MI355X-native Moco direct-collocation hot path (host side).

The product is libmocohip.so (C ABI, include/mocohip.h); this package is the
host-side mirror of the reference's MocoProblem / MocoSolver interface and
the model compiler that feeds the C ABI.
"""
from .model import (Axis, Bhargava2004Metabolics, Body, Coordinate, CoordinateActuator, DataTable,  # noqa: F401
                    DeGrooteFregly2016Muscle, ExternalForce, Function, Joint,
                    Model, PathPoint)
from .problem import (MocoAccelerationTrackingGoal, MocoAngularVelocityTrackingGoal, MocoBounds, MocoControlGoal,  # noqa: F401
                      MocoFinalTimeGoal, MocoJointReactionGoal, MocoOrientationTrackingGoal, MocoOutputGoal, MocoProblem, MocoStateTrackingGoal,
                      MocoSumSquaredStateGoal, MocoTranslationTrackingGoal)
from .solver import HipNLP, MocoHipSolver, MocoStudy  # noqa: F401
