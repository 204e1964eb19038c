// muscle_outputs.hip -- MocoOutputGoal over a DeGrooteFregly2016Muscle output
// (include/mocohip.h MH_GOAL_OUTPUT, enum mh_muscle_output) and
// mh_eval_muscle_outputs: a velocity-stage kernel.  Per thread (one goal at one
// lane) the poses and spatial velocities of the bodies its muscle's path
// touches, the path with its length and lengthening speed, and dgf_output
// (dae_device.hpp).  No
// Newton-Euler backward pass, no mass matrix, no dae_eval: the kernel works
// with prescribed kinematics and costs a fraction of a dynamics lane.  One
// instantiation per size class, selected by the context's whatever back end
// serves g and J.  A translation unit of its
// own, as joint_reaction.hip: generic.hip compiles to the code it had
// without it.
#include "mo_device.hpp"

// One thread per (goal of kind 17, grid point, lane), the goal slowest so that
// a wave works on one muscle, the lanes in the Lanes layout of k_eval (ND = NI
// - NSL + 2: the slack inputs get no lane): L = value / divisor of goal j of nmo
// (in goal order) to lv[(k stride + lane) nmo + j] where the lane's direction
// is live for the goal (mo_live; the base lane always); any other thread
// returns at once.  C (objective mode, base lanes only: stride 1):
// C[k ngoals + g] = quad[k] L.  The kinematic pass covers the bodies of the
// goal's muscle only; poses and velocities are indexed by body
// (dev_apply_wraps reads them so), in scratch for the larger size classes.
template <class Z>
__global__ void __launch_bounds__(64) k_muscle_outputs(DevModel M, Layout L, Lanes Ln, GoalSet GS, int nmo,
        const double* __restrict__ x, const double* __restrict__ grid, const double* __restrict__ quad,
        double* __restrict__ C, double* __restrict__ lv) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nlanes = (long)L.G * Ln.stride;
    if (gid >= nlanes * nmo) return;
    const int j = (int)(gid / nlanes);
    const long lane = gid - (long)j * nlanes;
    const int k = (int)(lane / Ln.stride);
    const int r = (int)(lane - (long)k * Ln.stride);
    const bool base = r == Ln.base;
    const int dir = r >= Ln.ND ? r - Ln.ND : r;
    int g = -1;
    for (int i = 0, n = 0; i < GS.ngoals && g < 0; ++i)
        if (GS.goals[i].kind == MH_GOAL_OUTPUT && n++ == j) g = i;
    if (g < 0) return;
    const int tb = GS.goals[g].term_begin, im = GS.gidx[tb], which = GS.gcol[tb];
    if (!base && !mo_live(M, im, which, dir)) return;
    PointIn in = point_in(L, x, k);
    const double t = lane_time(Ln, grid[k], x[0], x[1], r, in.pi, in.step);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    mo_with_kinematics<Z>(M, t, in, mo_muscle_bodies(M, im), X, V, [&](const auto& q, const auto& u) {
#pragma clang fp contract(off)
        double Lm, Sm;
        mo_path<Z::MP>(M, im, q, u, X, V, Lm, Sm);
        const double Lg = mo_value(M, im, which, Lm, Sm, in) / GS.gw[tb];
        lv[lane * nmo + j] = Lg;
        if (C) C[(long)k * GS.ngoals + g] = quad[k] * Lg;
    });
}

// The family's part of k_lane_goal_grad (goal_lanes.hpp): a direction is live
// for a goal where k_muscle_outputs evaluated its lane (mo_live).
struct MuscleOutputGoals : OneEntryPerGoal {
    static constexpr int kind = MH_GOAL_OUTPUT;
    struct Args {
        DevModel M;
    };
    __device__ static bool live(const Args& A, const GoalSet& GS, int g, int d) {
        const int tb = GS.goals[g].term_begin;
        return mo_live(A.M, GS.gidx[tb], GS.gcol[tb], d);
    }
};

// mh_eval_muscle_outputs: one thread per input row [time, NI point inputs],
// output which[o] of muscle mus[o] to outp[row nout + o]; one kinematic pass
// per row over the bodies of all the requested muscles.
template <class Z>
__global__ void __launch_bounds__(64) k_muscle_outputs_probe(DevModel M, Layout L, int nout,
        const int* __restrict__ mus, const int* __restrict__ which, int npts, const double* __restrict__ inp,
        double* __restrict__ outp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = inp + (long)p * (1 + L.NI);
    const PointIn in{row + 1, row + 1 + L.NS, row + 1 + L.NS + L.NC, L.NS, L.NC, -1, 0.0};
    unsigned long long mask = 0ull;
    for (int o = 0; o < nout; ++o) mask |= mo_muscle_bodies(M, mus[o]);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    mo_with_kinematics<Z>(M, row[0], in, mask, X, V, [&](const auto& q, const auto& u) {
        int last = -1;
        double Lm = 0.0, Sm = 0.0;
        for (int o = 0; o < nout; ++o) {
            if (mus[o] != last) {   // (consecutive outputs of one muscle share its path)
                last = mus[o];
                mo_path<Z::MP>(M, last, q, u, X, V, Lm, Sm);
            }
            outp[(long)p * nout + o] = mo_value(M, last, which[o], Lm, Sm, in);
        }
    });
}

template <class Z>
static void be_muscle_outputs(mh_ctx* c, const double* x, int mode) {
    const LaneGoals& R = c->lane_goals[LG_MUSCLE_OUTPUTS];
    launch_lane_goal_family<MuscleOutputGoals>(c, LG_MUSCLE_OUTPUTS, {c->M}, x, mode,
            [&](const Layout& L, const Lanes& ln, int mode) {
                const long threads = (long)c->G * ln.stride * R.entries;
                hipLaunchKernelGGL(k_muscle_outputs<Z>, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, c->stream,
                        c->M, L, ln, c->GS, R.entries, x, c->d_grid, c->d_quad, mode ? (double*)nullptr : c->d_C,
                        R.lv);
            });
}
template <class Z>
static void be_muscle_outputs_probe(mh_ctx* c, int nout, const int* mus, const int* which, int np,
        const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    hipLaunchKernelGGL(k_muscle_outputs_probe<Z>, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L, nout, mus,
            which, np, in, out);
}

const LaneGoalFamily& muscle_output_goals() {
    static const LaneGoalFamily kFamily = {
        MuscleOutputGoals::kind,
        {&be_muscle_outputs<SzSmall>, &be_muscle_outputs<SzMedium>, &be_muscle_outputs<SzLarge>,
         &be_muscle_outputs<SzBody>}};
    return kFamily;
}
void muscle_outputs_probe(mh_ctx* c, int nout, const int* mus, const int* which, int np, const double* in,
        double* out) {
    static constexpr decltype(&be_muscle_outputs_probe<SzSmall>) kProbe[4] = {
        &be_muscle_outputs_probe<SzSmall>, &be_muscle_outputs_probe<SzMedium>, &be_muscle_outputs_probe<SzLarge>,
        &be_muscle_outputs_probe<SzBody>};
    kProbe[c->size_class](c, nout, mus, which, np, in, out);
}
