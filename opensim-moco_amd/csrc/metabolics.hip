// metabolics.hip -- MocoOutputGoal over an output of a Bhargava2004Metabolics
// component (include/mocohip.h MH_GOAL_METABOLICS, enum mh_metabolics_output)
// and mh_eval_metabolics: velocity-stage kernels on muscle_outputs.hip's
// device functions (mo_device.hpp).  Per thread (one muscle of one goal at one
// lane) the poses and spatial velocities of the bodies the muscle's path
// touches, the path's length and lengthening speed, ONE evaluation of the
// muscle (dgf_outputs: all the quantities the model reads), then the muscle's
// activation, maintenance and shortening heat rates and its mechanical work
// rate.  The sum over a goal's muscles is taken by k_lane_goal_grad
// (goal_lanes.hpp) / k_metabolics_sum in the component's muscle order, one thread per value, so
// the result has the same bits on every run.  One instantiation per size
// class, selected by the context's whatever back end serves g and J.  A translation unit of its own, as muscle_outputs.hip.
#include "mo_device.hpp"

// Option flags of a component (goal_index of the block's first term).
enum {
    MET_SMOOTH = 1, MET_HUBER = 2, MET_FORCE_DEPENDENT = 4, MET_NEGATIVE_WORK = 8, MET_FORBID_NEGATIVE_POWER = 16,
    MET_MINIMUM_HEAT = 32
};

// A component's own numbers (the block's header terms).
struct MetHeader {
    int flags, output, channel;
    double divisor, basal, scale, vsmooth, psmooth, hsmooth;
};
__device__ __forceinline__ MetHeader met_header(const int* idx, const int* col, const double* w) {
    return MetHeader{idx[0], col[0], col[1], w[0], w[1], w[2], w[3], w[4], w[5]};
}

// The rates of one muscle (W): activation, maintenance and shortening heat,
// mechanical work, and the muscle's metabolic rate.
struct MetRates {
    double activation, maintenance, shortening, work, total;
};

// The model's switch between `left` (cond <= 0) and `right` (cond > 0)
// (Bhargava2004Metabolics.cpp:177-215): a step, its tanh blend, or the
// Huber-loss form, which blends the ramp (right - left) itself and so divides
// by cond; dir = +1 / -1: the side the ramp rises on.
__device__ __forceinline__ double met_step(double cond, double left, double right) {
    return cond <= 0.0 ? left : right;
}
__device__ __forceinline__ double met_tanh(double cond, double left, double right, double k) {
#pragma clang fp contract(off)
    const double b = 0.5 + 0.5 * tanh(k * cond);
    return left + (-left + right) * b;
}
__device__ __forceinline__ double met_huber(double cond, double left, double right, double k, int dir) {
#pragma clang fp contract(off)
    const double offset = dir == 1 ? left : right;
    const double scale = (right - left) / cond;
    const double state = dir * cond;
    const double shift = 0.5 * (1.0 / k);
    const double y = k * (state + shift);
    double f;
    if (y < 0.0) f = offset;
    else if (y <= 1.0) f = 0.5 * y * y + offset;
    else f = 1.0 * (y - 0.5 * 1.0) + offset;
    return scale * (f / k + offset * (1.0 - 1.0 / k));
}
__device__ __forceinline__ double met_cond(int flags, double cond, double left, double right, double k, int dir) {
    if (!(flags & MET_SMOOTH)) return met_step(cond, left, right);
    if (flags & MET_HUBER) return met_huber(cond, left, right, k, dir);
    return met_tanh(cond, left, right, k);
}

// The maintenance heat's dependence on the normalized fibre length: the
// piecewise-linear curve through (0, 0.5) (0.5, 0.5) (1, 1) (1.5, 0) (10, 0).
__device__ __forceinline__ double met_length_dependence(double nfl) {
#pragma clang fp contract(off)
    if (nfl <= 0.5) return 0.5;
    if (nfl <= 1.0) return 0.5 + (nfl - 0.5);
    if (nfl <= 1.5) return 1.0 - 2.0 * (nfl - 1.0);
    return 0.0;
}

// calcMetabolicRate (Bhargava2004Metabolics.cpp:337-537) for one muscle whose
// six terms are w (mass, slow-twitch ratio, activation constants slow / fast,
// maintenance constants slow / fast) from its quantities o, in the order the
// header (include/mocohip.h) fixes, every operation rounded on its own.
__device__ __forceinline__ MetRates met_rates(const MetHeader& H, const double* w, double Fmax, const DgfOut& o) {
#pragma clang fp contract(off)
    const double mass = w[0], ratio = w[1];
    const double act = H.scale * o.act, exc = H.scale * o.exc;
    const double Fpassive = o.passiveF, Factive = H.scale * o.activeF;
    const double Ftotal = Factive + Fpassive;
    const double v = o.fiberVelocity;
    const double half_pi = 1.5707963267948966;
    const double slow = ratio * sin(half_pi * exc);
    const double fast = (1.0 - ratio) * (1.0 - cos(half_pi * exc));
    const double Fiso = act * o.fAL * Fmax;
    MetRates R;
    R.activation = mass * (w[2] * slow + w[3] * fast);
    R.maintenance = mass * met_length_dependence(o.nfl) * (w[4] * slow + w[5] * fast);
    const double ve = v + 1e-16;
    double alpha;
    if (H.flags & MET_FORCE_DEPENDENT) {
        // (the tanh blend in both smooth modes: the two sides have different slopes)
        const double left = 0.16 * Fiso + 0.18 * Ftotal, right = 0.157 * Ftotal;
        alpha = (H.flags & MET_SMOOTH) ? met_tanh(ve, left, right, H.vsmooth) : met_step(ve, left, right);
    } else {
        alpha = met_cond(H.flags, ve, 0.25 * Ftotal, 0.0, H.vsmooth, -1);
    }
    R.shortening = -alpha * ve;
    if (H.flags & MET_NEGATIVE_WORK) R.work = -Factive * v;
    else R.work = met_cond(H.flags, ve, -Factive * v, 0.0, H.vsmooth, -1);
    if (H.flags & MET_FORBID_NEGATIVE_POWER) {
        const double before = R.activation + R.maintenance + R.shortening + R.work;
        if (H.flags & MET_SMOOTH) R.shortening -= met_cond(H.flags, -before, 0.0, before, H.psmooth, 1);
        else if (before < 0.0) R.shortening -= before;
    }
    double heat = R.activation + R.maintenance + R.shortening;
    if (H.flags & MET_MINIMUM_HEAT) {
        if (H.flags & MET_SMOOTH) heat = met_cond(H.flags, -heat + 1.0 * mass, heat, 1.0 * mass, H.hsmooth, 1);
        else if (heat < 1.0 * mass) heat = 1.0 * mass;
    }
    R.total = heat + R.work;
    return R;
}

// A muscle's contribution to output `which` of its component.
__device__ __forceinline__ double met_pick(const MetRates& R, int which) {
    switch (which) {
    case MH_MET_TOTAL_ACTIVATION_RATE: return R.activation;
    case MH_MET_TOTAL_MAINTENANCE_RATE: return R.maintenance;
    case MH_MET_TOTAL_SHORTENING_RATE: return R.shortening;
    case MH_MET_TOTAL_MECHANICAL_WORK_RATE: return R.work;
    default: return R.total;   // the total metabolic rate and one muscle's
    }
}

// Entry e of the nent muscle entries of all kind-18 goals (goal order, then
// the component's muscle order): its goal g, its position m among the goal's
// muscles and its position j among the kind-18 goals; false past the end.
__device__ __forceinline__ bool met_entry(const GoalSet& GS, int e, int& g, int& m) {
    for (int i = 0; i < GS.ngoals; ++i) {
        if (GS.goals[i].kind != MH_GOAL_METABOLICS) continue;
        const int nm = (GS.goals[i].term_count - MH_MET_HEADER) / MH_MET_PER_MUSCLE;
        if (e < nm) { g = i; m = e; return true; }
        e -= nm;
    }
    return false;
}

// Whether direction dir can change muscle im's rates: mo_live's rule with the
// excitation control always live (the model reads it beside the activation).
__device__ __forceinline__ bool met_live(const DevModel& M, int im, int dir) {
    return mo_live(M, im, MH_MO_EXCITATION, dir);
}

// One thread per (muscle entry, grid point, lane), the entries slowest so that
// a wave works on one muscle, the lanes in the Lanes layout of k_eval: the
// muscle's contribution to its goal's output (before the sum, the basal rate
// and the divisor) to lv[(k stride + lane) nent + e] where the lane's
// direction is live for the muscle (the base lane always).  Any other thread
// returns at once, as do the entries a per-muscle output does not name.
template <class Z>
__global__ void __launch_bounds__(64) k_metabolics(DevModel M, Layout L, Lanes Ln, GoalSet GS, int nent,
        const double* __restrict__ x, const double* __restrict__ grid, double* __restrict__ lv) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nlanes = (long)L.G * Ln.stride;
    if (gid >= nlanes * nent) return;
    const int e = (int)(gid / nlanes);
    const long lane = gid - (long)e * nlanes;
    const int k = (int)(lane / Ln.stride);
    const int r = (int)(lane - (long)k * Ln.stride);
    const bool base = r == Ln.base;
    const int dir = r >= Ln.ND ? r - Ln.ND : r;
    int g, m;
    if (!met_entry(GS, e, g, m)) return;
    const int tb = GS.goals[g].term_begin, mb = tb + MH_MET_HEADER + MH_MET_PER_MUSCLE * m;
    const MetHeader H = met_header(GS.gidx + tb, GS.gcol + tb, GS.gw + tb);
    if (H.output == MH_MET_MUSCLE_METABOLIC_RATE && m != H.channel) return;
    const int im = GS.gidx[mb];
    if (!base && !met_live(M, im, dir)) return;
    PointIn in = point_in(L, x, k);
    const double t = lane_time(Ln, grid[k], x[0], x[1], r, in.pi, in.step);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    mo_with_kinematics<Z>(M, t, in, mo_muscle_bodies(M, im), X, V, [&](const auto& q, const auto& u) {
        double Lm, Sm;
        mo_path<Z::MP>(M, im, q, u, X, V, Lm, Sm);
        const DgfOut o = mo_all(M, im, Lm, Sm, in);
        const MetRates R = met_rates(H, GS.gw + mb, M.mus[im].max_isometric_force, o);
        lv[lane * nent + e] = met_pick(R, H.output);
    });
}

// L of goal g (whose first entry is e0) at lane r of grid point k: the sum
// over its muscles, in order, of the lane's value -- the base lane's for a
// muscle the lane's direction cannot change, which has the bits an evaluation
// there would have --, the basal rate added for the total, over the divisor.
__device__ __forceinline__ double met_goal_value(const DevModel& M, const GoalSet& GS, const Lanes& Ln, int g,
        int e0, int nent, const double* __restrict__ lk, int r) {
#pragma clang fp contract(off)
    const mh_goal G = GS.goals[g];
    const int tb = G.term_begin, nm = (G.term_count - MH_MET_HEADER) / MH_MET_PER_MUSCLE;
    const MetHeader H = met_header(GS.gidx + tb, GS.gcol + tb, GS.gw + tb);
    const int dir = r >= Ln.ND ? r - Ln.ND : r;
    double s = 0.0;
    for (int m = 0; m < nm; ++m) {
        if (H.output == MH_MET_MUSCLE_METABOLIC_RATE && m != H.channel) continue;
        const int im = GS.gidx[tb + MH_MET_HEADER + MH_MET_PER_MUSCLE * m];
        const int rr = r == Ln.base || met_live(M, im, dir) ? r : Ln.base;
        s += lk[(long)rr * nent + e0 + m];
    }
    if (H.output == MH_MET_TOTAL_METABOLIC_RATE) s += H.basal;
    return s / H.divisor;
}

// Whether direction d can change goal g's value.
__device__ __forceinline__ bool met_goal_live(const DevModel& M, const GoalSet& GS, int g, int d) {
    if (d < 2) return true;
    const mh_goal G = GS.goals[g];
    const int tb = G.term_begin, nm = (G.term_count - MH_MET_HEADER) / MH_MET_PER_MUSCLE;
    const int output = GS.gcol[tb], channel = GS.gcol[tb + 1];
    for (int m = 0; m < nm; ++m) {
        if (output == MH_MET_MUSCLE_METABOLIC_RATE && m != channel) continue;
        if (met_live(M, GS.gidx[tb + MH_MET_HEADER + MH_MET_PER_MUSCLE * m], d)) return true;
    }
    return false;
}

// Objective mode, one thread per grid point (stride 1, base lanes only):
// C[k ngoals + g] = quad[k] L for every kind-18 goal.
__global__ void __launch_bounds__(64) k_metabolics_sum(DevModel M, Layout L, GoalSet GS, int nent,
        const double* __restrict__ quad, const double* __restrict__ lv, double* __restrict__ C) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L.G) return;
    const Lanes ln{MH_FD_FORWARD, 0, 1, 0, 0.0};
    int e0 = 0;
    for (int g = 0; g < GS.ngoals; ++g) {
        const mh_goal G = GS.goals[g];
        if (G.kind != MH_GOAL_METABOLICS) continue;
        C[(long)k * GS.ngoals + g] = quad[k] * met_goal_value(M, GS, ln, g, e0, nent, lv + (long)k * nent, 0);
        e0 += (G.term_count - MH_MET_HEADER) / MH_MET_PER_MUSCLE;
    }
}

// The family's part of k_lane_goal_grad (goal_lanes.hpp): a goal occupies one
// lane value per muscle and its value at a lane is their sum (met_goal_value);
// a direction is live for it where it is for one of its muscles.
struct MetabolicsGoals {
    static constexpr int kind = MH_GOAL_METABOLICS;
    struct Args {
        DevModel M;
    };
    __device__ static int entries(const mh_goal& G) { return (G.term_count - MH_MET_HEADER) / MH_MET_PER_MUSCLE; }
    __device__ static bool live(const Args& A, const GoalSet& GS, int g, int d) {
        return met_goal_live(A.M, GS, g, d);
    }
    __device__ static double value(const Args& A, const GoalSet& GS, const Lanes& Ln, int g,
            const double* __restrict__ lk, int nent, int e, int r) {
        return met_goal_value(A.M, GS, Ln, g, e, nent, lk, r);
    }
};

// mh_eval_metabolics: one thread per input row [time, NI point inputs]; the
// component's block (nm muscles) -> [total metabolic rate (with the basal
// rate), total activation, maintenance, shortening and work rates, each
// muscle's metabolic rate], the sums in the component's muscle order; one
// kinematic pass per row over the bodies of all its muscles.
template <class Z>
__global__ void __launch_bounds__(64) k_metabolics_probe(DevModel M, Layout L, int nm, const int* __restrict__ idx,
        const int* __restrict__ col, const double* __restrict__ w, int npts, const double* __restrict__ inp,
        double* __restrict__ outp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = inp + (long)p * (1 + L.NI);
    const PointIn in{row + 1, row + 1 + L.NS, row + 1 + L.NS + L.NC, L.NS, L.NC, -1, 0.0};
    const MetHeader H = met_header(idx, col, w);
    unsigned long long mask = 0ull;
    for (int m = 0; m < nm; ++m) mask |= mo_muscle_bodies(M, idx[MH_MET_HEADER + MH_MET_PER_MUSCLE * m]);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    double* out = outp + (long)p * (5 + nm);
    mo_with_kinematics<Z>(M, row[0], in, mask, X, V, [&](const auto& q, const auto& u) {
#pragma clang fp contract(off)
        double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < nm; ++m) {
            const int mb = MH_MET_HEADER + MH_MET_PER_MUSCLE * m, im = idx[mb];
            double Lm, Sm;
            mo_path<Z::MP>(M, im, q, u, X, V, Lm, Sm);
            const DgfOut o = mo_all(M, im, Lm, Sm, in);
            const MetRates R = met_rates(H, w + mb, M.mus[im].max_isometric_force, o);
            sum[0] += R.total; sum[1] += R.activation; sum[2] += R.maintenance; sum[3] += R.shortening;
            sum[4] += R.work;
            out[5 + m] = R.total;
        }
        out[0] = sum[0] + H.basal;
        for (int i = 1; i < 5; ++i) out[i] = sum[i];
    });
}

template <class Z>
static void be_metabolics(mh_ctx* c, const double* x, int mode) {
    const LaneGoals& R = c->lane_goals[LG_METABOLICS];
    launch_lane_goal_family<MetabolicsGoals>(c, LG_METABOLICS, {c->M}, x, mode,
            [&](const Layout& L, const Lanes& ln, int mode) {
                const long threads = (long)c->G * ln.stride * R.entries;
                hipLaunchKernelGGL(k_metabolics<Z>, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, c->stream,
                        c->M, L, ln, c->GS, R.entries, x, c->d_grid, R.lv);
                if (mode == 0)   // objective mode: the goals' sums over their muscles
                    hipLaunchKernelGGL(k_metabolics_sum, dim3((unsigned)((c->G + 63) / 64)), dim3(64), 0, c->stream,
                            c->M, L, c->GS, R.entries, c->d_quad, R.lv, c->d_C);
            });
}
template <class Z>
static void be_metabolics_probe(mh_ctx* c, int nm, const int* idx, const int* col, const double* w, int np,
        const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    hipLaunchKernelGGL(k_metabolics_probe<Z>, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L, nm, idx, col, w,
            np, in, out);
}

const LaneGoalFamily& metabolics_goals() {
    static const LaneGoalFamily kFamily = {
        MetabolicsGoals::kind,
        {&be_metabolics<SzSmall>, &be_metabolics<SzMedium>, &be_metabolics<SzLarge>, &be_metabolics<SzBody>}};
    return kFamily;
}
void metabolics_probe(mh_ctx* c, int nm, const int* idx, const int* col, const double* w, int np, const double* in,
        double* out) {
    static constexpr decltype(&be_metabolics_probe<SzSmall>) kProbe[4] = {
        &be_metabolics_probe<SzSmall>, &be_metabolics_probe<SzMedium>, &be_metabolics_probe<SzLarge>,
        &be_metabolics_probe<SzBody>};
    kProbe[c->size_class](c, nm, idx, col, w, np, in, out);
}
