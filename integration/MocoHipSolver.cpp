/* MocoHipSolver.cpp — see MocoHipSolver.h.  NOT compiled in this repository
 * (OpenSim and Ipopt are absent from the image); written
 * against opensim-core b0222c2's public headers and Ipopt 3.12.8.
 *
 * Pieces, each mirroring the reference function it replaces:
 *   compileProblemRep    the Model / MocoProblemRep walk (MocoProblemRep.h:
 *                        69-116) into mhb::Problem: the same rules as the
 *                        Python lowering of .osim files (mocohip/osim.py,
 *                        model.py, problem.py), whose tapes the C++ builder
 *                        reproduces byte for byte (tests/test_builder.py);
 *   solveImpl            MocoCasADiSolver::solveImpl (MocoCasADiSolver.cpp:
 *                        312-415): guess -> iterate, the NLP on the GPU
 *                        through the C ABI, Ipopt over it (mh_ipopt_tnlp.hpp),
 *                        the iterate back to a MocoSolution, setSolutionStats
 *                        (MocoSolver.h:97-102).
 */
#include "MocoHipSolver.h"

#include <OpenSim/Actuators/CoordinateActuator.h>
#include <OpenSim/Actuators/SpringGeneralizedForce.h>
#include <OpenSim/Common/Constant.h>
#include <OpenSim/Common/GCVSpline.h>
#include <OpenSim/Common/GCVSplineSet.h>
#include <OpenSim/Common/LinearFunction.h>
#include <OpenSim/Common/MultiplierFunction.h>
#include <OpenSim/Common/PiecewiseLinearFunction.h>
#include <OpenSim/Common/SimmSpline.h>
#include <OpenSim/Common/Stopwatch.h>
#include <OpenSim/Moco/Components/Bhargava2004Metabolics.h>
#include <OpenSim/Moco/Components/DeGrooteFregly2016Muscle.h>
#include <OpenSim/Moco/Components/PositionMotion.h>
#include <OpenSim/Moco/MocoGoal/MocoControlGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoInitialActivationGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoMarkerFinalGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoMarkerTrackingGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoAccelerationTrackingGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoAngularVelocityTrackingGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoJointReactionGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoOrientationTrackingGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoOutputGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoTranslationTrackingGoal.h>
#include <OpenSim/Simulation/StatesTrajectory.h>
#include <OpenSim/Moco/MocoGoal/MocoStateTrackingGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoSumSquaredStateGoal.h>
#include <OpenSim/Moco/MocoGoal/MocoGoal.h>
#include <OpenSim/Moco/MocoControlBoundConstraint.h>
#include <OpenSim/Moco/MocoFrameDistanceConstraint.h>
#include <OpenSim/Moco/MocoProblemRep.h>
#include <OpenSim/Moco/MocoUtilities.h>
#include <OpenSim/Simulation/Model/ExternalForce.h>
#include <OpenSim/Simulation/Model/Station.h>
#include <Moco/Components/StationPlaneContactForce.h>
#include <OpenSim/Simulation/Model/Model.h>
#include <OpenSim/Simulation/Model/PhysicalOffsetFrame.h>
#include <OpenSim/Simulation/SimbodyEngine/CoordinateCouplerConstraint.h>
#include <OpenSim/Simulation/SimbodyEngine/CustomJoint.h>
#include <OpenSim/Simulation/SimbodyEngine/PinJoint.h>
#include <OpenSim/Simulation/SimbodyEngine/SliderJoint.h>
#include <OpenSim/Simulation/SimbodyEngine/WeldJoint.h>
#include <OpenSim/Simulation/Wrap/PathWrap.h>
#include <OpenSim/Simulation/Wrap/WrapCylinder.h>
#include <OpenSim/Simulation/Model/ConditionalPathPoint.h>
#include <OpenSim/Simulation/Model/MovingPathPoint.h>

#include "mh_ipopt_tnlp.hpp"
#include "mh_trajectory.hpp"

using namespace OpenSim;

namespace {

// ---- functions -------------------------------------------------------------
// OpenSim functions of one coordinate -> mhb::Function (osim.py
// parse_function): Constant, LinearFunction, SimmSpline, and a
// MultiplierFunction scaling either.
mhb::Function toFunction(const Function& f, const std::string& coord) {
    mhb::Function out;
    out.coord = coord;
    if (const auto* c = dynamic_cast<const Constant*>(&f)) {
        out.kind = MH_FN_CONSTANT;
        out.a = c->getValue();
        out.coord.clear();
    } else if (const auto* l = dynamic_cast<const LinearFunction*>(&f)) {
        out.kind = MH_FN_LINEAR;
        out.a = l->getSlope();
        out.b = l->getIntercept();
    } else if (const auto* s = dynamic_cast<const SimmSpline*>(&f)) {
        out.kind = MH_FN_SIMMSPLINE;
        const int n = s->getSize();
        for (int i = 0; i < n; ++i) {
            out.x.push_back(s->getX()[i]);
            out.y.push_back(s->getY()[i]);
        }
    } else if (const auto* m = dynamic_cast<const MultiplierFunction*>(&f)) {
        out = toFunction(m->getFunction(), coord);
        out.scale *= m->getScale();
    } else {
        OPENSIM_THROW(Exception, "MocoHipSolver: function type '{}' is not supported "
                                 "(Constant, LinearFunction, SimmSpline, MultiplierFunction)",
                f.getConcreteClassName());
    }
    return out;
}

// A data table as the piecewise polynomial the device evaluates: the
// GCVSplineSet the reference builds over it (GCVSplineSet(table, labels,
// degree), the splines of ExternalForce, MocoStateTrackingGoal and
// PositionMotion) converted exactly -- on [t_s, t_{s+1}] a degree-d spline
// is its Taylor polynomial at t_s, coefficient k = f^(k)(t_s) / k!.
mhb::Table toTable(const std::string& name, const TimeSeriesTable& table, int degree,
        const std::vector<std::string>& renamed = {}) {
    const auto labels = table.getColumnLabels();
    GCVSplineSet splines(table, labels, degree);
    const auto& time = table.getIndependentColumn();
    mhb::Table out;
    out.name = name;
    out.degree = degree;
    out.columns = renamed.empty() ? labels : renamed;
    out.breaks.assign(time.begin(), time.end());
    const int nseg = (int)time.size() - 1;
    const int ncol = (int)labels.size();
    out.coefs.assign((size_t)nseg * ncol * (degree + 1), 0.0);
    for (int s = 0; s < nseg; ++s) {
        const SimTK::Vector t(1, time[s]);
        for (int c = 0; c < ncol; ++c) {
            const auto& sp = *splines.getGCVSpline(c);
            double fact = 1.0;
            for (int k = 0; k <= degree; ++k) {
                if (k > 0) fact *= k;
                const double v = k == 0 ? sp.calcValue(t)
                                        : sp.calcDerivative(std::vector<int>(k, 0), t);
                out.coefs[((size_t)s * ncol + c) * (degree + 1) + k] = v / fact;
            }
        }
    }
    return out;
}

// ---- frames ----------------------------------------------------------------
// A joint frame: the body it is attached to and its offset (translation,
// body-fixed XYZ orientation), identity for a body / ground frame itself.
void frameOf(const PhysicalFrame& f, std::string& body, double loc[3], double orient[3]) {
    for (int i = 0; i < 3; ++i) loc[i] = orient[i] = 0.0;
    if (const auto* o = dynamic_cast<const PhysicalOffsetFrame*>(&f)) {
        body = o->getParentFrame().findBaseFrame().getName();
        for (int i = 0; i < 3; ++i) {
            loc[i] = o->get_translation()[i];
            orient[i] = o->get_orientation()[i];
        }
    } else {
        body = f.findBaseFrame().getName();
    }
}

mhb::Coordinate toCoordinate(const Coordinate& c) {
    mhb::Coordinate out;
    out.name = c.getName();
    out.range[0] = c.getRangeMin();
    out.range[1] = c.getRangeMax();
    out.motion_type = c.getMotionType() == Coordinate::Translational ? "translational" : "rotational";
    out.default_value = c.getDefaultValue();
    out.path = c.getAbsolutePathString();
    return out;
}

// Joint -> axes (osim.py _axes_for): Pin = rotation about the child frame's
// z, Slider = translation along x, Weld = none, CustomJoint = its
// SpatialTransform's rotations then translations.
mhb::Joint toJoint(const Joint& j) {
    mhb::Joint out;
    out.name = j.getName();
    frameOf(j.getParentFrame(), out.parent, out.loc_in_parent, out.orient_in_parent);
    std::string child;
    frameOf(j.getChildFrame(), child, out.loc_in_child, out.orient_in_child);
    out.child = child;
    for (int i = 0; i < j.numCoordinates(); ++i) out.coordinates.push_back(toCoordinate(j.get_coordinates(i)));
    auto linear = [](const std::string& coord) {
        mhb::Function f;
        f.kind = MH_FN_LINEAR;
        f.coord = coord;
        f.a = 1.0;
        return f;
    };
    if (dynamic_cast<const PinJoint*>(&j)) {
        mhb::Axis a;
        a.type = MH_AXIS_ROTATION;
        a.func = linear(out.coordinates.at(0).name);
        out.axes.push_back(a);
    } else if (dynamic_cast<const SliderJoint*>(&j)) {
        mhb::Axis a;
        a.type = MH_AXIS_TRANSLATION;
        a.dir[0] = 1; a.dir[1] = 0; a.dir[2] = 0;
        a.func = linear(out.coordinates.at(0).name);
        out.axes.push_back(a);
    } else if (dynamic_cast<const WeldJoint*>(&j)) {
        // no axes
    } else if (const auto* cj = dynamic_cast<const CustomJoint*>(&j)) {
        const SpatialTransform& st = cj->getSpatialTransform();
        for (int i = 0; i < 6; ++i) {
            const TransformAxis& ta = st.getTransformAxis(i);
            const auto names = ta.getCoordinateNames();
            OPENSIM_THROW_IF(names.size() > 1, Exception,
                    "MocoHipSolver: TransformAxis of joint '{}' with more than one coordinate", j.getName());
            const std::string coord = names.size() ? names[0] : std::string();
            mhb::Axis a;
            a.type = i < 3 ? MH_AXIS_ROTATION : MH_AXIS_TRANSLATION;
            for (int d = 0; d < 3; ++d) a.dir[d] = ta.getAxis()[d];
            a.func = ta.hasFunction() ? toFunction(ta.getFunction(), coord) : mhb::Function{};
            OPENSIM_THROW_IF(coord.empty() && a.func.kind != MH_FN_CONSTANT, Exception,
                    "MocoHipSolver: non-constant TransformAxis without a coordinate in '{}'", j.getName());
            out.axes.push_back(a);
        }
    } else {
        OPENSIM_THROW(Exception, "MocoHipSolver: joint type '{}' is not supported",
                j.getConcreteClassName());
    }
    return out;
}

// ---- muscles and paths -------------------------------------------------------
mhb::Muscle toMuscle(const DeGrooteFregly2016Muscle& m) {
    mhb::Muscle out;
    out.name = m.getName();
    out.path = m.getAbsolutePathString();
    out.max_isometric_force = m.get_max_isometric_force();
    out.optimal_fiber_length = m.get_optimal_fiber_length();
    out.tendon_slack_length = m.get_tendon_slack_length();
    out.pennation_angle_at_optimal = m.get_pennation_angle_at_optimal();
    out.max_contraction_velocity = m.get_max_contraction_velocity();
    out.activation_time_constant = m.get_activation_time_constant();
    out.deactivation_time_constant = m.get_deactivation_time_constant();
    out.default_activation = m.get_default_activation();
    out.default_normalized_tendon_force = m.get_default_normalized_tendon_force();
    out.active_force_width_scale = m.get_active_force_width_scale();
    out.fiber_damping = m.get_fiber_damping();
    out.passive_fiber_strain_at_one_norm_force = m.get_passive_fiber_strain_at_one_norm_force();
    out.tendon_strain_at_one_norm_force = m.get_tendon_strain_at_one_norm_force();
    out.ignore_passive_fiber_force = m.get_ignore_passive_fiber_force();
    out.ignore_activation_dynamics = m.get_ignore_activation_dynamics();
    out.ignore_tendon_compliance = m.get_ignore_tendon_compliance();
    out.tendon_compliance_dynamics_mode = m.get_tendon_compliance_dynamics_mode();
    out.min_control = m.getMinControl();
    out.max_control = m.getMaxControl();
    const GeometryPath& gp = m.getGeometryPath();
    const PathPointSet& pps = gp.getPathPointSet();
    for (int i = 0; i < pps.getSize(); ++i) {
        const AbstractPathPoint& ap = pps.get(i);
        mhb::PathPoint p;
        p.name = ap.getName();
        p.body = ap.getParentFrame().findBaseFrame().getName();
        if (const auto* mp = dynamic_cast<const MovingPathPoint*>(&ap)) {
            p.kind = MH_PP_MOVING;
            if (mp->hasXLocation()) p.fx = toFunction(mp->get_x_location(), mp->getXCoordinate().getName());
            if (mp->hasYLocation()) p.fy = toFunction(mp->get_y_location(), mp->getYCoordinate().getName());
            if (mp->hasZLocation()) p.fz = toFunction(mp->get_z_location(), mp->getZCoordinate().getName());
        } else if (const auto* cp = dynamic_cast<const ConditionalPathPoint*>(&ap)) {
            p.kind = MH_PP_CONDITIONAL;
            for (int d = 0; d < 3; ++d) p.loc[d] = cp->get_location()[d];
            p.coord = cp->getCoordinate().getName();
            p.range[0] = cp->get_range(0);
            p.range[1] = cp->get_range(1);
        } else if (const auto* fp = dynamic_cast<const PathPoint*>(&ap)) {
            p.kind = MH_PP_FIXED;
            for (int d = 0; d < 3; ++d) p.loc[d] = fp->get_location()[d];
        } else {
            OPENSIM_THROW(Exception, "MocoHipSolver: path point type '{}' of '{}' is not supported",
                    ap.getConcreteClassName(), m.getName());
        }
        out.points.push_back(p);
    }
    // PathWrapSet (the muscles DeGrooteFregly2016Muscle::replaceMuscles
    // creates carry none: it copies the PathPointSet only,
    // DeGrooteFregly2016Muscle.cpp:1007-1020)
    const PathWrapSet& ws = gp.getWrapSet();
    for (int i = 0; i < ws.getSize(); ++i) {
        const PathWrap& w = ws.get(i);
        mhb::PathWrapRef r;
        r.wrap = w.getWrapObjectName();
        r.range_begin = w.getStartPoint();
        r.range_end = w.getEndPoint();
        out.path_wraps.push_back(r);
    }
    return out;
}

// ---- the model ---------------------------------------------------------------
void compileModel(const Model& model, mhb::Problem& prob) {
    mhb::Model& m = prob.model;
    m.name = model.getName();
    const SimTK::Vec3 g = model.getGravity();
    for (int i = 0; i < 3; ++i) m.gravity[i] = g[i];
    for (const Body& b : model.getComponentList<Body>()) {
        mhb::Body hb;
        hb.name = b.getName();
        hb.mass = b.getMass();
        for (int i = 0; i < 3; ++i) hb.com[i] = b.getMassCenter()[i];
        const SimTK::Inertia I = b.getInertia();
        for (int i = 0; i < 3; ++i) {
            hb.inertia[i] = I.getMoments()[i];
            hb.inertia[3 + i] = I.getProducts()[i];
        }
        m.add_body(hb);
        for (const WrapObject& w : b.getComponentList<WrapObject>()) {
            const auto* wc = dynamic_cast<const WrapCylinder*>(&w);
            OPENSIM_THROW_IF(!wc, Exception, "MocoHipSolver: wrap object '{}' ({}) is not a WrapCylinder",
                    w.getName(), w.getConcreteClassName());
            mhb::WrapCylinder hw;
            hw.name = wc->getName();
            hw.body = b.getName();
            hw.radius = wc->get_radius();
            hw.length = wc->get_length();
            for (int d = 0; d < 3; ++d) {
                hw.xyz_body_rotation[d] = wc->get_xyz_body_rotation()[d];
                hw.translation[d] = wc->get_translation()[d];
            }
            hw.quadrant = wc->get_quadrant();
            hw.active = wc->get_active();
            m.add_wrap(hw);
        }
    }
    for (const Joint& j : model.getComponentList<Joint>()) m.add_joint(toJoint(j));
    // actuators in force-set order (MocoUtilities.cpp:557-587)
    for (const Actuator& a : model.getComponentList<Actuator>()) {
        if (!a.get_appliesForce()) continue;
        if (const auto* mu = dynamic_cast<const DeGrooteFregly2016Muscle*>(&a)) {
            m.add_muscle(toMuscle(*mu));
        } else if (const auto* ca = dynamic_cast<const CoordinateActuator*>(&a)) {
            mhb::CoordinateActuator hc;
            hc.name = ca->getName();
            hc.path = ca->getAbsolutePathString();
            hc.coordinate = ca->getCoordinate()->getName();
            hc.optimal_force = ca->getOptimalForce();
            hc.min_control = ca->getMinControl();
            hc.max_control = ca->getMaxControl();
            m.add_coordinate_actuator(hc);
        } else {
            OPENSIM_THROW(Exception, "MocoHipSolver: actuator '{}' of type '{}' is not supported "
                                     "(DeGrooteFregly2016Muscle, CoordinateActuator)",
                    a.getName(), a.getConcreteClassName());
        }
    }
    // SpringGeneralizedForces (-stiffness (q - rest_length) - viscosity u on
    // their coordinate; testMocoParameters.cpp:50-55)
    for (const SpringGeneralizedForce& f : model.getComponentList<SpringGeneralizedForce>()) {
        if (!f.get_appliesForce()) continue;
        mhb::SpringGeneralizedForce hs;
        hs.name = f.getName();
        hs.path = f.getAbsolutePathString();
        hs.coordinate = f.get_coordinate();
        hs.stiffness = f.getStiffness();
        hs.rest_length = f.getRestLength();
        hs.viscosity = f.getViscosity();
        m.add_spring(hs);
    }
    // ExternalForces on ground-expressed data (ModOpAddExternalLoads): one
    // table per data source, cubic GCV splines as ExternalForce builds them
    int ntab = 0;
    for (const ExternalForce& ef : model.getComponentList<ExternalForce>()) {
        OPENSIM_THROW_IF(ef.get_force_expressed_in_body() != "ground" || ef.get_point_expressed_in_body() != "ground",
                Exception, "MocoHipSolver: ExternalForce '{}' must be expressed in ground", ef.getName());
        const Storage& data = ef.getDataSource();
        TimeSeriesTable tt = data.exportToTable();
        const std::string tname = "grf" + std::to_string(ntab++);
        m.add_table(toTable(tname, tt, 3));
        mhb::ExternalForce he;
        he.name = ef.getName();
        he.body = ef.get_applied_to_body();
        he.table = tname;
        he.force_identifier = ef.get_force_identifier();
        he.point_identifier = ef.get_point_identifier();
        he.torque_identifier = ef.get_torque_identifier();
        m.add_external_force(he);
    }
    // station-plane contact forces (StationPlaneContactForce.h): the station
    // and the class's properties, in component-list order; mh_create runs
    // them on the generic interpreter (the plane is ground y = 0, friction
    // along ground x, as in the reference).  SmoothSphereHalfSpaceForce is not
    // a StationPlaneContactForce and stays refused with every other force.
    for (const StationPlaneContactForce& cf : model.getComponentList<StationPlaneContactForce>()) {
        if (!cf.get_appliesForce()) continue;
        const auto& st = cf.getConnectee<Station>("station");
        mhb::Station hs;
        hs.name = st.getName();
        hs.path = st.getAbsolutePathString();
        hs.body = st.getParentFrame().findBaseFrame().getName();
        const SimTK::Vec3 loc = st.getParentFrame().findTransformInBaseFrame() * st.get_location();
        for (int d = 0; d < 3; ++d) hs.location[d] = loc[d];
        m.add_station(hs);
        mhb::ContactForce hc;
        hc.name = cf.getName();
        hc.path = cf.getAbsolutePathString();
        hc.station = hs.path;
        if (const auto* a = dynamic_cast<const AckermannVanDenBogert2010Force*>(&cf)) {
            hc.kind = MH_EXT_CONTACT_ACKERMANN_VAN_DEN_BOGERT;
            const double p[5] = {a->get_stiffness(), a->get_dissipation(), a->get_friction_coefficient(),
                    a->get_tangent_velocity_scaling_factor(), 0.0};
            std::copy(p, p + 5, hc.params);
        } else if (const auto* e = dynamic_cast<const EspositoMiller2018Force*>(&cf)) {
            hc.kind = MH_EXT_CONTACT_ESPOSITO_MILLER;
            const double p[5] = {e->get_stiffness(), e->get_dissipation(), e->get_friction_coefficient(),
                    e->get_tangent_velocity_scaling_factor(), e->get_depth_offset()};
            std::copy(p, p + 5, hc.params);
        } else if (const auto* f = dynamic_cast<const MeyerFregly2016Force*>(&cf)) {
            hc.kind = MH_EXT_CONTACT_MEYER_FREGLY;   // friction coefficient 1, latch velocity 0.05: fixed there
            const double p[5] = {f->get_stiffness(), f->get_dissipation(), 1.0, 0.05, f->get_tscale()};
            std::copy(p, p + 5, hc.params);
        } else {
            OPENSIM_THROW(Exception, "MocoHipSolver: StationPlaneContactForce '{}' of class {} is not supported",
                    cf.getName(), cf.getConcreteClassName());
        }
        m.add_contact_force(hc);
    }
    for (const Marker& mk : model.getComponentList<Marker>()) {
        mhb::Marker hm;
        hm.name = mk.getName();
        hm.path = mk.getAbsolutePathString();
        hm.body = mk.getParentFrame().findBaseFrame().getName();
        for (int d = 0; d < 3; ++d) hm.location[d] = mk.get_location()[d];
        m.add_marker(hm);
    }
    for (const CoordinateCouplerConstraint& k : model.getComponentList<CoordinateCouplerConstraint>()) {
        if (!k.isEnforced(model.getWorkingState())) continue;
        const auto ind = k.getIndependentCoordinateNames();
        OPENSIM_THROW_IF(ind.size() != 1, Exception,
                "MocoHipSolver: CoordinateCouplerConstraint '{}' with {} independent coordinates",
                k.getName(), ind.size());
        mhb::CoordinateCoupler hk;
        hk.name = k.getName();
        hk.dependent = k.getDependentCoordinateName();
        hk.function = toFunction(k.getFunction(), ind[0]);
        hk.scale_factor = k.get_scale_factor();
        m.add_constraint(hk);
    }
}

mhb::Bounds toBounds(const MocoBounds& b) {
    mhb::Bounds out;
    if (b.isSet()) {
        out.lower = b.getLower();
        out.upper = b.getUpper();
    }
    return out;
}

mhb::BoundFunction toBoundFunction(const Function& f) {
    mhb::BoundFunction out;
    if (const auto* c = dynamic_cast<const Constant*>(&f)) {
        out.kind = mhb::BoundFunction::CONSTANT;
        out.value = c->getValue();
    } else if (const auto* p = dynamic_cast<const PiecewiseLinearFunction*>(&f)) {
        out.kind = mhb::BoundFunction::PIECEWISE_LINEAR;
        for (int i = 0; i < p->getSize(); ++i) {
            out.x.push_back(p->getX(i));
            out.y.push_back(p->getY(i));
        }
    } else if (const auto* s = dynamic_cast<const GCVSpline*>(&f)) {
        // the spline over its own knots as a piecewise polynomial (toTable)
        TimeSeriesTable t;
        t.setColumnLabels({"bound"});
        for (int i = 0; i < s->getSize(); ++i) t.appendRow(s->getX()[i], SimTK::RowVector(1, s->getY()[i]));
        const mhb::Table tb = toTable("bound", t, s->getDegree());
        out.kind = mhb::BoundFunction::SPLINE;
        out.x = tb.breaks;
        out.breaks = tb.breaks;
        out.coefs = tb.coefs;
        out.degree = tb.degree;
    } else {
        OPENSIM_THROW(Exception, "MocoHipSolver: bound function '{}' is not supported", f.getConcreteClassName());
    }
    return out;
}

}  // namespace

// ---- compileProblemRep --------------------------------------------------------
mhb::Problem OpenSim::compileProblemRep(const MocoProblemRep& rep) {
    mhb::Problem prob;
    const Model& model = rep.getModelBase();
    compileModel(model, prob);
    prob.time_initial = toBounds(rep.getTimeInitialBounds());
    prob.time_final = toBounds(rep.getTimeFinalBounds());
    for (const std::string& n : rep.createStateInfoNames()) {
        const MocoVariableInfo& vi = rep.getStateInfo(n);
        prob.state_infos.push_back({n, {toBounds(vi.getBounds()), toBounds(vi.getInitialBounds()),
                                        toBounds(vi.getFinalBounds())}});
    }
    for (const std::string& n : rep.createControlInfoNames()) {
        const MocoVariableInfo& vi = rep.getControlInfo(n);
        prob.control_infos.push_back({n, {toBounds(vi.getBounds()), toBounds(vi.getInitialBounds()),
                                          toBounds(vi.getFinalBounds())}});
    }
    // prescribed kinematics (MocoInverse's PositionMotion, MocoInverse.cpp:
    // 46-66): its coordinate functions as one table, columns = value paths
    if (rep.isPrescribedKinematics()) {
        const auto& pm = model.getComponentList<PositionMotion>().begin();
        TimeSeriesTable samples;
        std::vector<std::string> cols;
        const auto coords = model.getCoordinatesInMultibodyTreeOrder();
        // sample each coordinate's function at its own knots (GCVSplines of
        // a common time column, PositionMotion::createFromTable)
        const FunctionSet& fs = pm->get_functions();
        const auto* first = dynamic_cast<const GCVSpline*>(&fs.get(0));
        OPENSIM_THROW_IF(!first, Exception, "MocoHipSolver: PositionMotion functions must be GCVSplines");
        std::vector<std::string> labels;
        for (int i = 0; i < fs.getSize(); ++i) labels.push_back(fs.get(i).getName());
        samples.setColumnLabels(labels);
        for (int r = 0; r < first->getSize(); ++r) {
            SimTK::RowVector row(fs.getSize());
            for (int i = 0; i < fs.getSize(); ++i) row[i] = dynamic_cast<const GCVSpline&>(fs.get(i)).getY()[r];
            samples.appendRow(first->getX()[r], row);
        }
        prob.position_motion = toTable("kinematics", samples, first->getDegree());
    }
    // goals: costs, then the endpoint constraints (MocoProblemRep::
    // createEndpointConstraintNames order)
    auto addGoal = [&](const MocoGoal& g) {
        mhb::Goal hg;
        hg.name = g.getName();
        hg.weight = g.getWeight();
        if (const auto* c = dynamic_cast<const MocoControlGoal*>(&g)) {
            hg.kind = mhb::Goal::CONTROL;
            hg.exponent = c->getExponent();
            const MocoWeightSet& ws = c->get_control_weights();
            for (int i = 0; i < ws.getSize(); ++i) hg.weights.push_back({ws.get(i).getName(), ws.get(i).getWeight()});
        } else if (const auto* s = dynamic_cast<const MocoStateTrackingGoal*>(&g)) {
            hg.kind = mhb::Goal::STATE_TRACKING;
            TimeSeriesTable ref = s->getReference().process(&model);
            hg.table = "state_reference_" + g.getName();
            prob.model.add_table(toTable(hg.table, ref, 5));
            const MocoWeightSet& ws = s->get_states_weight_set();
            for (int i = 0; i < ws.getSize(); ++i) hg.weights.push_back({ws.get(i).getName(), ws.get(i).getWeight()});
        } else if (dynamic_cast<const MocoFinalTimeGoal*>(&g)) {
            hg.kind = mhb::Goal::FINAL_TIME;
        } else if (const auto* q = dynamic_cast<const MocoSumSquaredStateGoal*>(&g)) {
            hg.kind = mhb::Goal::SUM_SQUARED_STATE;
            const MocoWeightSet& ws = q->get_state_weights();
            for (int i = 0; i < ws.getSize(); ++i) hg.weights.push_back({ws.get(i).getName(), ws.get(i).getWeight()});
        } else if (dynamic_cast<const MocoInitialActivationGoal*>(&g)) {
            hg.kind = mhb::Goal::INITIAL_ACTIVATION;
            hg.mode = g.getModeAsString() == "cost" ? "cost" : "endpoint_constraint";
        } else if (const auto* mf = dynamic_cast<const MocoMarkerFinalGoal*>(&g)) {
            hg.kind = mhb::Goal::MARKER_FINAL;
            hg.point_name = mf->get_point_name();
            for (int d = 0; d < 3; ++d) hg.reference_location[d] = mf->get_reference_location()[d];
        } else if (const auto* mt = dynamic_cast<const MocoMarkerTrackingGoal*>(&g)) {
            // the flattened marker table (columns <label>_1, _2, _3) as a
            // model table, splined as GCVSplineSet(table) does (degree 5);
            // the labels with their weights by reference index --
            // mhb::make_rep runs initializeOnModelImpl's checks.  (A
            // reference given as a marker file is expected to be loaded:
            // the goal loads it in initializeOnModelImpl, which has run on
            // this MocoProblemRep.)
            hg.kind = mhb::Goal::MARKER_TRACKING;
            const MarkersReference& mref = mt->getMarkersReference();
            hg.table = "markers_reference_" + g.getName();
            // (the goal has a setter only, and its property accessors are
            // protected: read the property by name)
            hg.allow_unused_references = mt->getPropertyByName("allow_unused_references").getValue<bool>();
            const auto& names = mref.getNames();
            SimTK::Array_<double> weights;
            mref.getWeights(model.getWorkingState(), weights);
            for (int i = 0; i < (int)names.size(); ++i) hg.weights.push_back({names[i], weights[i]});
            std::vector<std::string> sorted(names.begin(), names.end());
            std::sort(sorted.begin(), sorted.end());
            // (a redundant label cannot be flattened; make_rep reports it)
            if (std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end())
                prob.model.add_table(toTable(hg.table, mref.getMarkerTable().flatten(), 5));
        } else if (dynamic_cast<const MocoTranslationTrackingGoal*>(&g) ||
                   dynamic_cast<const MocoOrientationTrackingGoal*>(&g) ||
                   dynamic_cast<const MocoAngularVelocityTrackingGoal*>(&g) ||
                   dynamic_cast<const MocoAccelerationTrackingGoal*>(&g)) {
            // The goals keep their splines and an in-memory reference table
            // private, so the frame data is computed again from what is
            // public: the states reference (as initializeOnModelImpl does,
            // MocoOrientationTrackingGoal.cpp:74-109) or the reference file.
            // frame_paths follows the documented behaviour (empty: every
            // column), not the inverted test of the reference's code
            // (DESIGN.md).  The flattened table -- <path>/position_x|y|z,
            // <path>/quaternion_e0..3 or <path>/angular_velocity_x|y|z (the
            // last realized to the velocity stage, MocoAngularVelocityTracking
            // Goal.cpp:98-111) -- goes in as a model table, splined as
            // GCVSplineSet(table) does (degree 5); the frames as offset
            // frames with their orientation; mhb::make_rep runs the checks.
            // A MocoAccelerationTrackingGoal (<path>/acceleration_x|y|z) has a
            // reference file only: the class has no states_reference property.
            const bool accel = dynamic_cast<const MocoAccelerationTrackingGoal*>(&g) != nullptr;
            const bool orient = dynamic_cast<const MocoOrientationTrackingGoal*>(&g) != nullptr;
            const bool angvel = dynamic_cast<const MocoAngularVelocityTrackingGoal*>(&g) != nullptr;
            hg.kind = orient ? mhb::Goal::ORIENTATION_TRACKING
                    : (angvel ? mhb::Goal::ANGULAR_VELOCITY_TRACKING
                              : (accel ? mhb::Goal::ACCELERATION_TRACKING : mhb::Goal::TRANSLATION_TRACKING));
            const std::string what =
                    orient ? "rotation" : (angvel ? "angular_velocity" : (accel ? "acceleration" : "translation"));
            hg.table = what + "_reference_" + g.getName();
            const auto& pathsProp = g.getPropertyByName("frame_paths");
            std::vector<std::string> paths;
            for (int i = 0; i < pathsProp.size(); ++i) paths.push_back(pathsProp.getValue<std::string>(i));
            const std::string file = g.getPropertyByName(what + "_reference_file").getValue<std::string>();
            OPENSIM_THROW_IF(accel && file.empty(), Exception,
                    "MocoHipSolver: goal '{}': an acceleration reference set in memory cannot be read back from the "
                    "goal; give it as a file", g.getName());
            const TableProcessor noStates;
            const auto& statesRef =
                    accel ? noStates : g.getPropertyByName("states_reference").getValue<TableProcessor>();
            std::vector<double> times;
            std::vector<std::vector<SimTK::Rotation>> rotations;   // [row][frame]
            std::vector<std::vector<SimTK::Vec3>> positions;       // or angular velocities
            if (!file.empty()) {
                auto select = [&](const std::vector<std::string>& labels) {
                    if (paths.empty()) paths = labels;
                    std::vector<int> cols;
                    for (const auto& path : paths) {
                        auto it = std::find(labels.begin(), labels.end(), path);
                        OPENSIM_THROW_IF(it == labels.end(), Exception,
                                "Expected frame_paths to match one of the column labels in the {} reference, but "
                                "frame path '{}' not found in the reference labels.",
                                orient ? "rotation"
                                       : (angvel ? "angular velocity" : (accel ? "acceleration" : "translation")),
                                path);
                        cols.push_back((int)(it - labels.begin()));
                    }
                    return cols;
                };
                if (orient) {
                    TimeSeriesTable_<SimTK::Rotation> t(file);
                    const auto cols = select(t.getColumnLabels());
                    for (int r = 0; r < (int)t.getNumRows(); ++r) {
                        times.push_back(t.getIndependentColumn()[r]);
                        rotations.emplace_back();
                        for (int c : cols) rotations.back().push_back(t.getRowAtIndex(r)[c]);
                    }
                } else {
                    TimeSeriesTableVec3 t(file);
                    const auto cols = select(t.getColumnLabels());
                    for (int r = 0; r < (int)t.getNumRows(); ++r) {
                        times.push_back(t.getIndependentColumn()[r]);
                        positions.emplace_back();
                        for (int c : cols) positions.back().push_back(t.getRowAtIndex(r)[c]);
                    }
                }
            } else {
                OPENSIM_THROW_IF(statesRef.empty(), Exception,
                        "MocoHipSolver: goal '{}': a reference table set in memory cannot be read back from the goal; "
                        "give it as a file or as a states reference", g.getName());
                OPENSIM_THROW_IF(paths.empty(), Exception,
                        "Expected paths in the frame_paths property, but none were found.");
                TimeSeriesTable states = statesRef.process("", &model);
                checkLabelsMatchModelStates(model, states.getColumnLabels());
                auto traj = StatesTrajectory::createFromStatesStorage(model, convertTableToStorage(states));
                for (auto state : traj) {
                    if (angvel) model.realizeVelocity(state);
                    else model.realizePosition(state);
                    times.push_back(state.getTime());
                    rotations.emplace_back();
                    positions.emplace_back();
                    for (const auto& path : paths) {
                        const Frame& f = model.getComponent<Frame>(path);
                        rotations.back().push_back(f.getRotationInGround(state));
                        positions.back().push_back(angvel ? f.getAngularVelocityInGround(state)
                                                          : f.getPositionInGround(state));
                    }
                }
            }
            const int per = orient ? 4 : 3;
            std::vector<std::string> labels;
            static const char* const psfx[3] = {"position_x", "position_y", "position_z"};
            static const char* const wsfx[3] = {"angular_velocity_x", "angular_velocity_y", "angular_velocity_z"};
            static const char* const asfx[3] = {"acceleration_x", "acceleration_y", "acceleration_z"};
            for (const auto& path : paths)
                for (int c = 0; c < per; ++c)
                    labels.push_back(orient ? path + "/quaternion_e" + std::to_string(c)
                                            : path + "/" + (angvel ? wsfx[c] : (accel ? asfx[c] : psfx[c])));
            TimeSeriesTable flat;
            std::vector<std::string> sorted(paths);
            std::sort(sorted.begin(), sorted.end());
            // (a redundant label cannot be a column twice; make_rep reports it)
            if (std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end()) {
                flat.setColumnLabels(labels);
                for (size_t r = 0; r < times.size(); ++r) {
                    SimTK::RowVector row((int)labels.size());
                    for (size_t i = 0; i < paths.size(); ++i) {
                        if (orient) {
                            const auto e = rotations[r][i].convertRotationToQuaternion();
                            for (int c = 0; c < 4; ++c) row[(int)i * 4 + c] = e[c];
                        } else {
                            for (int c = 0; c < 3; ++c) row[(int)i * 3 + c] = positions[r][i][c];
                        }
                    }
                    flat.appendRow(times[r], row);
                }
                prob.model.add_table(toTable(hg.table, flat, 5));
            }
            const auto& ws = g.getPropertyByName(what + "_weights").getValue<MocoWeightSet>();
            for (const auto& path : paths) {
                hg.weights.push_back({path, ws.contains(path) ? ws.get(path).getWeight() : 1.0});
                if (!model.hasComponent<Frame>(path)) continue;   // make_rep: no frame
                const Frame& f = model.getComponent<Frame>(path);
                const Frame& base = f.findBaseFrame();
                const SimTK::Transform X_BO = f.findTransformInBaseFrame();
                const SimTK::Vec3 xyz = X_BO.R().convertRotationToBodyFixedXYZ();
                mhb::OffsetFrame of;
                of.name = path;
                of.path = path;
                of.body = &base == &model.getGround() ? "ground" : base.getName();
                for (int d = 0; d < 3; ++d) {
                    of.translation[d] = X_BO.p()[d];
                    of.orientation[d] = xyz[d];
                }
                prob.model.add_offset_frame(of);
            }
        } else if (dynamic_cast<const MocoJointReactionGoal*>(&g)) {
            // the properties as they are (the goal has setters only: read by
            // name); the joint by its name (mhb::make_rep
            // resolves /jointset/<name> or the name) and the expressed-in
            // frame as an offset frame of its base frame with its orientation.
            // mhb::make_rep runs initializeOnModelImpl's checks and computes
            // the denominator (total mass x |gravity|) from the lowered model.
            hg.kind = mhb::Goal::JOINT_REACTION;
            hg.joint_path = g.getPropertyByName("joint_path").getValue<std::string>();
            if (!hg.joint_path.empty() && model.hasComponent<Joint>(hg.joint_path))
                hg.joint_path = model.getComponent<Joint>(hg.joint_path).getName();
            hg.loads_frame = g.getPropertyByName("loads_frame").getValue<std::string>();
            hg.expressed_in_frame_path = g.getPropertyByName("expressed_in_frame_path").getValue<std::string>();
            const auto& measures = g.getPropertyByName("reaction_measures");
            for (int i = 0; i < measures.size(); ++i) hg.reaction_measures.push_back(measures.getValue<std::string>(i));
            const auto& ws = g.getPropertyByName("reaction_weights").getValue<MocoWeightSet>();
            for (int i = 0; i < ws.getSize(); ++i) hg.weights.push_back({ws.get(i).getName(), ws.get(i).getWeight()});
            const std::string& path = hg.expressed_in_frame_path;
            if (!path.empty() && model.hasComponent<Frame>(path)) {   // (else make_rep: no frame)
                const Frame& f = model.getComponent<Frame>(path);
                const Frame& base = f.findBaseFrame();
                const SimTK::Transform X_BO = f.findTransformInBaseFrame();
                const SimTK::Vec3 xyz = X_BO.R().convertRotationToBodyFixedXYZ();
                mhb::OffsetFrame of;
                of.name = path;
                of.path = path;
                of.body = &base == &model.getGround() ? "ground" : base.getName();
                for (int d = 0; d < 3; ++d) {
                    of.translation[d] = X_BO.p()[d];
                    of.orientation[d] = xyz[d];
                }
                prob.model.add_offset_frame(of);
            }
        } else if (dynamic_cast<const MocoOutputGoal*>(&g)) {
            // an output of a DeGrooteFregly2016Muscle (include/mocohip.h enum
            // mh_muscle_output; <muscle path>|<output>, or its GeometryPath's
            // length / lengthening_speed): the component and the output's name
            // are checked here.  divide_by_displacement needs
            // calcSystemDisplacement.
            hg.kind = mhb::Goal::OUTPUT;
            hg.output_path = g.getPropertyByName("output_path").getValue<std::string>();
            hg.divide_by_mass = g.getPropertyByName("divide_by_mass").getValue<bool>();
            hg.divide_by_displacement = g.getPropertyByName("divide_by_displacement").getValue<bool>();
            OPENSIM_THROW_IF(hg.divide_by_displacement, Exception,
                    "MocoHipSolver: goal '{}': MocoOutputGoal with divide_by_displacement is not supported",
                    g.getName());
            OPENSIM_THROW_IF(hg.output_path.empty(), Exception, "No output_path provided.");
            std::string comp = hg.output_path.substr(0, hg.output_path.find('|'));
            if (model.hasComponent<Bhargava2004Metabolics>(comp)) {
                // an output of a Bhargava2004Metabolics: the component travels
                // with the goal (mhb::MetabolicsComponent; make_rep lowers it to
                // MH_GOAL_METABOLICS and checks the output's name and channel).
                // The path handed on is /<name>|<output>, the form make_rep
                // matches, wherever the component sits in the model.
                const auto& met = model.getComponent<Bhargava2004Metabolics>(comp);
                mhb::MetabolicsComponent& mc = hg.metabolics;
                hg.has_metabolics = true;
                mc.name = met.getName();
                hg.output_path = "/" + mc.name + hg.output_path.substr(hg.output_path.find('|'));
                mc.enforce_minimum_heat_rate_per_muscle = met.get_enforce_minimum_heat_rate_per_muscle();
                mc.use_force_dependent_shortening_prop_constant =
                        met.get_use_force_dependent_shortening_prop_constant();
                mc.basal_coefficient = met.get_basal_coefficient();
                mc.basal_exponent = met.get_basal_exponent();
                mc.muscle_effort_scaling_factor = met.get_muscle_effort_scaling_factor();
                mc.include_negative_mechanical_work = met.get_include_negative_mechanical_work();
                mc.forbid_negative_total_power = met.get_forbid_negative_total_power();
                mc.use_smoothing = met.get_use_smoothing();
                mc.smoothing_type = met.get_smoothing_type();
                mc.velocity_smoothing = met.get_velocity_smoothing();
                mc.power_smoothing = met.get_power_smoothing();
                mc.heat_rate_smoothing = met.get_heat_rate_smoothing();
                for (int i = 0; i < met.getProperty_muscle_parameters().size(); ++i) {
                    const auto& p = met.get_muscle_parameters(i);
                    const auto* dgf = dynamic_cast<const DeGrooteFregly2016Muscle*>(&p.getMuscle());
                    OPENSIM_THROW_IF(!dgf, Exception,
                            "MocoHipSolver: goal '{}': muscle '{}' of '{}' is not a DeGrooteFregly2016Muscle",
                            g.getName(), p.getName(), comp);
                    mhb::MetabolicsMuscle mp;
                    mp.name = p.getName();
                    mp.muscle_path = dgf->getAbsolutePathString();
                    mp.ratio_slow_twitch_fibers = p.get_ratio_slow_twitch_fibers();
                    mp.specific_tension = p.get_specific_tension();
                    mp.density = p.get_density();
                    mp.activation_constant_slow_twitch = p.get_activation_constant_slow_twitch();
                    mp.activation_constant_fast_twitch = p.get_activation_constant_fast_twitch();
                    mp.maintenance_constant_slow_twitch = p.get_maintenance_constant_slow_twitch();
                    mp.maintenance_constant_fast_twitch = p.get_maintenance_constant_fast_twitch();
                    if (p.get_use_provided_muscle_mass()) mp.muscle_mass = p.get_provided_muscle_mass();
                    mc.muscles.push_back(mp);
                }
                prob.goals.push_back(hg);
                return;
            }
            const std::string gp = "/geometrypath";
            if (comp.size() >= gp.size() && comp.compare(comp.size() - gp.size(), gp.size(), gp) == 0)
                comp.resize(comp.size() - gp.size());
            OPENSIM_THROW_IF(!model.hasComponent<DeGrooteFregly2016Muscle>(comp), Exception,
                    "MocoHipSolver: goal '{}': output '{}' is not an output of a DeGrooteFregly2016Muscle; only "
                    "those are supported (include/mocohip.h enum mh_muscle_output)",
                    g.getName(), hg.output_path);
            const size_t bar = hg.output_path.find('|');
            OPENSIM_THROW_IF(bar == std::string::npos || mhb::muscle_output_id(hg.output_path.substr(bar + 1)) < 0,
                    Exception,
                    "MocoHipSolver: goal '{}': output '{}' is not a supported output of a DeGrooteFregly2016Muscle "
                    "(include/mocohip.h enum mh_muscle_output)",
                    g.getName(), hg.output_path);
        } else {
            OPENSIM_THROW(Exception, "MocoHipSolver: goal '{}' of type '{}' is not supported (SURVEY §8 A11)",
                    g.getName(), g.getConcreteClassName());
        }
        prob.goals.push_back(hg);
    };
    for (int i = 0; i < rep.getNumCosts(); ++i) addGoal(rep.getCostByIndex(i));
    for (int i = 0; i < rep.getNumEndpointConstraints(); ++i) addGoal(rep.getEndpointConstraintByIndex(i));
    // path constraints: MocoControlBoundConstraint and MocoFrameDistanceConstraint,
    // in the problem's order
    for (int i = 0; i < rep.getNumPathConstraints(); ++i) {
        const MocoPathConstraint& pc = rep.getPathConstraintByIndex(i);
        if (const auto* fdc = dynamic_cast<const MocoFrameDistanceConstraint*>(&pc)) {
            // each frame as an offset frame of its base frame (a body or
            // ground) under the frame's own path: only its origin matters;
            // mhb::make_rep runs initializeOnModelImpl's checks
            mhb::FrameDistanceConstraint hc;
            hc.name = fdc->getName();
            hc.projection = fdc->get_projection();
            if (!fdc->getProperty_projection_vector().empty())
                for (int d = 0; d < 3; ++d) hc.projection_vector.push_back(fdc->get_projection_vector()[d]);
            const auto& pairs = fdc->getProperty_frame_pairs();
            for (int k = 0; k < pairs.size(); ++k) {
                const MocoFrameDistanceConstraintPair& fp = pairs.getValue(k);
                mhb::FrameDistancePair hp;
                hp.frame1_path = fp.get_frame1_path();
                hp.frame2_path = fp.get_frame2_path();
                hp.minimum_distance = fp.get_minimum_distance();
                hp.maximum_distance = fp.get_maximum_distance();
                for (const std::string& path : {hp.frame1_path, hp.frame2_path}) {
                    if (!model.hasComponent<Frame>(path)) continue;   // make_rep: "Could not find frame"
                    const Frame& f = model.getComponent<Frame>(path);
                    const Frame& base = f.findBaseFrame();
                    const SimTK::Vec3 loc = f.findTransformInBaseFrame().p();
                    mhb::OffsetFrame of;
                    of.name = path;
                    of.path = path;
                    of.body = &base == &model.getGround() ? "ground" : base.getName();
                    for (int d = 0; d < 3; ++d) of.translation[d] = loc[d];
                    prob.model.add_offset_frame(of);
                }
                hc.frame_pairs.push_back(hp);
            }
            prob.add_path_constraint(hc);
            continue;
        }
        const auto* cb = dynamic_cast<const MocoControlBoundConstraint*>(&pc);
        OPENSIM_THROW_IF(!cb, Exception, "MocoHipSolver: path constraint '{}' of type '{}' is not supported",
                pc.getName(), pc.getConcreteClassName());
        mhb::ControlBoundConstraint hc;
        hc.name = cb->getName();
        for (const auto& p : cb->getControlPaths()) hc.control_paths.push_back(p);
        if (cb->hasLowerBound()) hc.lower = toBoundFunction(cb->getLowerBound());
        if (cb->hasUpperBound()) hc.upper = toBoundFunction(cb->getUpperBound());
        hc.equality_with_lower = cb->getEqualityWithLower();
        prob.add_path_constraint(hc);
    }
    // MocoParameters in createParameterNames order (the x layout's last
    // block); mhb::make_rep resolves the component paths and properties and
    // throws MocoParameter::initializeOnModel's errors for the rest (a
    // property this build does not parameterize, e.g. optimal_fiber_length,
    // is refused there by name)
    for (const std::string& name : rep.createParameterNames()) {
        const MocoParameter& par = rep.getParameter(name);
        mhb::Parameter hp;
        hp.name = name;
        hp.component_paths = par.getComponentPaths();
        hp.property_name = par.getPropertyName();
        hp.bounds = toBounds(par.getBounds());
        hp.property_element = par.getProperty_property_element().size() ? par.get_property_element() : -1;
        prob.parameters.push_back(hp);
    }
    return prob;
}

// ---- the solver ----------------------------------------------------------------
MocoHipSolver::MocoHipSolver() { constructProperties(); }

void MocoHipSolver::constructProperties() {
    constructProperty_optim_finite_difference_scheme("central");
    constructProperty_optim_sparsity_detection("none");
    constructProperty_device(0);
    constructProperty_jacobian_mode("callback-fd");
}

mhb::SolverSettings MocoHipSolver::settings() const {
    mhb::SolverSettings s;
    s.num_mesh_intervals = get_num_mesh_intervals();
    s.transcription_scheme = get_transcription_scheme();
    s.interpolate_control_midpoints = get_interpolate_control_midpoints();
    s.optim_finite_difference_scheme = get_optim_finite_difference_scheme();
    s.device = get_device();
    s.multibody_dynamics_mode = get_multibody_dynamics_mode();
    s.implicit_multibody_acceleration_bounds[0] = get_implicit_multibody_acceleration_bounds().getLower();
    s.implicit_multibody_acceleration_bounds[1] = get_implicit_multibody_acceleration_bounds().getUpper();
    s.implicit_auxiliary_derivative_bounds[0] = get_implicit_auxiliary_derivative_bounds().getLower();
    s.implicit_auxiliary_derivative_bounds[1] = get_implicit_auxiliary_derivative_bounds().getUpper();
    s.enforce_constraint_derivatives = get_enforce_constraint_derivatives();
    s.minimize_lagrange_multipliers = get_minimize_lagrange_multipliers();
    s.lagrange_multiplier_weight = get_lagrange_multiplier_weight();
    s.velocity_correction_bounds[0] = get_velocity_correction_bounds().getLower();
    s.velocity_correction_bounds[1] = get_velocity_correction_bounds().getUpper();
    s.jacobian_mode = get_jacobian_mode();
    s.optim_sparsity_detection = get_optim_sparsity_detection();
    s.optim_sparsity_detection_random_count = 3;   // MocoCasADiSolver.cpp:251
    return s;
}

void MocoHipSolver::setGuess(MocoTrajectory guess) {
    clearGuess();
    m_guessFromAPI = std::move(guess);
}
void MocoHipSolver::setGuessFile(const std::string& file) {
    clearGuess();
    set_guess_file(file);
}
void MocoHipSolver::clearGuess() {
    m_guessFromAPI = MocoTrajectory();
    m_guessFromFile = MocoTrajectory();
    set_guess_file("");
    m_guessToUse.reset();
}
const MocoTrajectory& MocoHipSolver::getGuess() const {
    if (!m_guessToUse) {
        if (get_guess_file() != "" && m_guessFromFile.getRef().empty()) {
            m_guessFromFile = MocoTrajectory(get_guess_file());
            m_guessToUse.reset(&m_guessFromFile.getRef());
        } else if (!m_guessFromAPI.empty()) {
            m_guessToUse.reset(&m_guessFromAPI);
        } else {
            m_guessToUse.reset(&m_guessFromFile.getRef());   // empty: the bounds guess
        }
    }
    return m_guessToUse.getRef();
}

namespace {

// The trajectory conversions of the reference (MocoCasOCProblem.h:70-187:
// convertToCasOCIterate / convertToMocoTrajectory) over every variable block
// by name -- states, controls, multipliers, derivatives, slacks -- shared
// with the command-line path (csrc/host/mh_trajectory.hpp; mh_build
// --solution writes the same MocoSolution as a .sto, tests/
// test_trajectory_cpp.py checks it against the Python conversion and the
// reference's MocoInverse solution file).
mhb::TrajectoryTable toTable(const MocoTrajectory& t) {
    mhb::TrajectoryTable T;
    const SimTK::Vector time = t.getTime();
    for (int k = 0; k < time.size(); ++k) T.time.push_back(time[k]);
    auto take = [&](const std::vector<std::string>& names, const SimTK::Matrix& M, std::vector<std::string>& tn,
                    std::vector<double>& td) {
        tn = names;
        td.assign((size_t)M.nrow() * M.ncol(), 0.0);
        for (int k = 0; k < M.nrow(); ++k)
            for (int j = 0; j < M.ncol(); ++j) td[(size_t)k * M.ncol() + j] = M(k, j);
    };
    take(t.getStateNames(), t.getStatesTrajectory(), T.state_names, T.states);
    take(t.getControlNames(), t.getControlsTrajectory(), T.control_names, T.controls);
    take(t.getMultiplierNames(), t.getMultipliersTrajectory(), T.multiplier_names, T.multipliers);
    take(t.getDerivativeNames(), t.getDerivativesTrajectory(), T.derivative_names, T.derivatives);
    take(t.getSlackNames(), t.getSlacksTrajectory(), T.slack_names, T.slacks);
    T.parameter_names = t.getParameterNames();
    const SimTK::RowVector& pv = t.getParameters();
    for (int j = 0; j < pv.size(); ++j) T.parameters.push_back(pv[j]);
    return T;
}

// The guess resampled at the grid times (CasOCTranscription.cpp:593-597),
// then every block it names into the iterate; unnamed blocks stay 0.
std::vector<double> toIterate(MocoTrajectory guess, const mhb::ProblemRep& hrep, const mh_options& o) {
    const auto t = guess.getTime();
    const auto times = mhb::grid_times(o, t[0], t[t.size() - 1]);
    guess.resample(SimTK::Vector((int)times.size(), times.data()));
    return mhb::trajectory_to_iterate(toTable(guess), hrep, o);
}

// The solution iterate as a MocoSolution at the grid times, every block by
// name; the slacks appended the reference's way (convertToMocoTrajectory:
// the N interval values placed uniformly over [t0, tf] and interpolated
// onto the grid).
MocoSolution toSolution(const std::vector<double>& x, const mhb::ProblemRep& hrep, const mh_options& o) {
    const mhb::TrajectoryTable T = mhb::iterate_to_trajectory(x, hrep, o);
    const int G = (int)T.time.size();
    auto matrix = [&](const std::vector<double>& d, size_t nv) {
        SimTK::Matrix M(G, (int)nv);
        for (int k = 0; k < G; ++k)
            for (size_t j = 0; j < nv; ++j) M(k, (int)j) = d[(size_t)k * nv + j];
        return M;
    };
    SimTK::RowVector parameters((int)T.parameters.size());
    for (int j = 0; j < parameters.size(); ++j) parameters[j] = T.parameters[(size_t)j];
    MocoSolution sol(SimTK::Vector(G, T.time.data()), T.state_names, T.control_names, T.multiplier_names,
            T.derivative_names, T.parameter_names, matrix(T.states, T.state_names.size()),
            matrix(T.controls, T.control_names.size()), matrix(T.multipliers, T.multiplier_names.size()),
            matrix(T.derivatives, T.derivative_names.size()), parameters);
    const int N = o.num_mesh_intervals;
    const int nsl = (int)T.slack_names.size();
    if (nsl) {
        const SimTK::Vector slackTime = createVectorLinspace(N, T.time.front(), T.time.back());
        for (int l = 0; l < nsl; ++l) {
            SimTK::Vector v(N);
            for (int i = 0; i < N; ++i) v[i] = T.slacks[(size_t)(2 * i + 1) * nsl + l];   // the midpoints
            sol.appendSlack(T.slack_names[l], interpolate(slackTime, v, sol.getTime()));
        }
    }
    return sol;
}

// Ipopt's return status by name (IpReturnCodes_inc.h), as MocoCasADiSolver
// reports CasADi's "return_status".
std::string ipoptStatusName(Ipopt::ApplicationReturnStatus s) {
    switch (s) {
    case Ipopt::Solve_Succeeded: return "Solve_Succeeded";
    case Ipopt::Solved_To_Acceptable_Level: return "Solved_To_Acceptable_Level";
    case Ipopt::Infeasible_Problem_Detected: return "Infeasible_Problem_Detected";
    case Ipopt::Search_Direction_Becomes_Too_Small: return "Search_Direction_Becomes_Too_Small";
    case Ipopt::Diverging_Iterates: return "Diverging_Iterates";
    case Ipopt::User_Requested_Stop: return "User_Requested_Stop";
    case Ipopt::Feasible_Point_Found: return "Feasible_Point_Found";
    case Ipopt::Maximum_Iterations_Exceeded: return "Maximum_Iterations_Exceeded";
    case Ipopt::Restoration_Failed: return "Restoration_Failed";
    case Ipopt::Error_In_Step_Computation: return "Error_In_Step_Computation";
    case Ipopt::Maximum_CpuTime_Exceeded: return "Maximum_CpuTime_Exceeded";
    case Ipopt::Not_Enough_Degrees_Of_Freedom: return "Not_Enough_Degrees_Of_Freedom";
    case Ipopt::Invalid_Problem_Definition: return "Invalid_Problem_Definition";
    case Ipopt::Invalid_Option: return "Invalid_Option";
    case Ipopt::Invalid_Number_Detected: return "Invalid_Number_Detected";
    default: return "Ipopt status " + std::to_string((int)s);
    }
}

// The context owned for the solve: destroyed on every exit path.
struct CtxGuard {
    mh_ctx* ctx = nullptr;
    ~CtxGuard() { mh_destroy(ctx); }
};

}  // namespace

MocoSolution MocoHipSolver::solveImpl() const {
    const Stopwatch stopwatch;
    const MocoProblemRep& rep = getProblemRep();
    if (get_verbosity()) {
        log_info(std::string(72, '='));
        log_info("MocoHipSolver starting (MI355X direct-collocation hot path).");
        rep.printDescription();
    }
    // lower the problem and transcribe it on the device
    const mhb::Problem prob = compileProblemRep(rep);
    mhb::ProblemRep hrep;
    mhb::make_rep(prob, hrep);
    mh_options opt = mhb::make_options(settings());
    // the starting point: the user's guess resampled on the grid, every
    // block by name, else the bounds-midpoint guess (MocoCasADiSolver.cpp:
    // 326-332); "initial-guess" sparsity detection probes at it
    // (CasOCSolver.cpp:74-76; null: the bounds midpoint, the same guess)
    std::vector<double> x0;
    const MocoTrajectory& guess = getGuess();
    if (!guess.empty()) x0 = toIterate(guess, hrep, opt);
    // the library's n before mh_create reads the guess (n doubles): the
    // host-only layout query, so a layout mismatch is an error, not a read
    // past the iterate
    mh_nlp_info layout{};
    OPENSIM_THROW_IF(mh_get_nlp_info_for(&hrep.problem, &opt, &layout) != MH_OK, Exception,
            "MocoHipSolver: {}", mh_last_error());
    OPENSIM_THROW_IF(!x0.empty() && (int64_t)x0.size() != layout.n, Exception,
            "MocoHipSolver: the guess iterate has {} values, the problem has n = {}", x0.size(), layout.n);
    if (opt.sparsity_detection == MH_SPARSITY_INITIAL_GUESS) opt.sparsity_guess = x0.empty() ? nullptr : x0.data();
    CtxGuard ctx;
    OPENSIM_THROW_IF(mh_create(&hrep.problem, &opt, &ctx.ctx) != MH_OK, Exception,
            "MocoHipSolver: mh_create failed: {}", mh_last_error());
    Ipopt::SmartPtr<mocohip::MocoHipTNLP> tnlp = new mocohip::MocoHipTNLP(ctx.ctx, x0);
    mocohip::IpoptSettings ips;
    ips.verbosity = get_verbosity();
    ips.optim_max_iterations = get_optim_max_iterations();
    ips.optim_convergence_tolerance = get_optim_convergence_tolerance();
    ips.optim_constraint_tolerance = get_optim_constraint_tolerance();
    ips.optim_hessian_approximation = get_optim_hessian_approximation();
    ips.optim_ipopt_print_level = get_optim_ipopt_print_level();
    const Ipopt::ApplicationReturnStatus status = mocohip::solve(tnlp, ips);
    MocoSolution solution = toSolution(tnlp->solution(), hrep, opt);
    // the objective's terms at the solution, one per cost goal
    // (MocoCasADiSolver.cpp:395-402: the solution's objective breakdown)
    std::vector<std::pair<std::string, double>> breakdown;
    const std::vector<std::string> costs = rep.createCostNames();
    std::vector<double> terms(costs.size() + 1, 0.0);
    int32_t nterms = (int32_t)terms.size();
    if (mh_eval_objective_terms(ctx.ctx, tnlp->solution().data(), terms.data(), &nterms) == MH_OK)
        for (int i = 0; i < (int)costs.size() && i < nterms; ++i) breakdown.emplace_back(costs[i], terms[i]);
    const long long elapsed = stopwatch.getElapsedTimeInNs();
    const bool success = status == Ipopt::Solve_Succeeded || status == Ipopt::Solved_To_Acceptable_Level;
    setSolutionStats(solution, success, tnlp->objective(), ipoptStatusName(status), tnlp->iterations(),
            SimTK::nsToSec(elapsed), breakdown);
    if (get_verbosity()) {
        log_info("Elapsed real time: {}.", stopwatch.formatNs(elapsed));
        log_info(std::string(72, '='));
    }
    return solution;
}
