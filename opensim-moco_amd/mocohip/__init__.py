"""mocohip — MI355X-native Moco direct-collocation hot path (host side).

The product is libmocohip.so (C ABI, include/mocohip.h); this package is the
host-side mirror of the reference's MocoProblem / MocoSolver interface and
the model compiler that feeds the C ABI.
"""
from .model import (AckermannVanDenBogert2010Force, Axis, Bhargava2004Metabolics, Body, Coordinate,  # noqa: F401
                    CoordinateActuator, DataTable, DeGrooteFregly2016Muscle, EspositoMiller2018Force, ExternalForce,
                    Function, Joint, MeyerFregly2016Force, Model, PathPoint, Station)
from .problem import (MocoAccelerationTrackingGoal, MocoAngularVelocityTrackingGoal, MocoBounds, MocoControlGoal,  # noqa: F401
                      MocoFinalTimeGoal, MocoJointReactionGoal, MocoOrientationTrackingGoal, MocoOutputGoal, MocoProblem, MocoStateTrackingGoal,
                      MocoSumSquaredStateGoal, MocoTranslationTrackingGoal)
from .solver import HipNLP, MocoHipSolver, MocoStudy  # noqa: F401
