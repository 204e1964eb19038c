// joint_reaction.hip -- MocoJointReactionGoal's kernels (include/mocohip.h
// MH_GOAL_JOINT_REACTION): the generic interpreter (dae_device.hpp) run with
// the point's accelerations per finite-difference lane, and the joint load
// read from its workspace.  One instantiation per size class, selected by
// the context's size class whatever back end serves g and J.
#include "goal_lanes.hpp"

// ---- MocoJointReactionGoal (include/mocohip.h MH_GOAL_JOINT_REACTION) -------
// The reaction load r (moment x, y, z, force x, y, z) of goal G from the
// workspace of a dae_eval run with the point's accelerations: F[b + 1] after
// the backward pass is what b's inboard joint transmits to b, in ground, about
// the ground origin.  Steps 2 and 3 of the header, operation for operation.
template <class W>
__device__ __forceinline__ void joint_reaction_load(const DevModel& M, const W& w, const GoalSet& GS,
        const mh_goal& G, double* r) {
#pragma clang fp contract(off)
    const int tb = G.term_begin;
    const int b = GS.gidx[tb], e = GS.gcol[tb];
    const double* Reo = GS.gw + tb;
    const bool child = GS.gcol[tb + 15] == 1;
    const mh_body& B = M.bodies[b];
    const SV& F = w.F[b + 1];
    const Pose& Po = w.X[child ? b + 1 : B.parent + 1];
    const double* lo = child ? B.p_BM : B.p_PF;
    double o[3];
    for (int i = 0; i < 3; ++i)
        o[i] = Po.p[i] + ((Po.R[3 * i] * lo[0] + Po.R[3 * i + 1] * lo[1]) + Po.R[3 * i + 2] * lo[2]);
    const double f0 = F.v0, f1 = F.v1, f2 = F.v2;
    const double c0 = o[1] * f2 - o[2] * f1, c1 = o[2] * f0 - o[0] * f2, c2 = o[0] * f1 - o[1] * f0;
    double ld[6] = {F.w0 - c0, F.w1 - c1, F.w2 - c2, f0, f1, f2};
    if (!child)
        for (int i = 0; i < 6; ++i) ld[i] = -ld[i];
    double Rge[9];
    if (e >= 0) {
        const double* A = w.X[e + 1].R;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Rge[3 * i + j] = (A[3 * i] * Reo[j] + A[3 * i + 1] * Reo[3 + j]) + A[3 * i + 2] * Reo[6 + j];
    } else {
        for (int i = 0; i < 9; ++i) Rge[i] = Reo[i];
    }
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < 3; ++i)
            r[3 * h + i] = (Rge[i] * ld[3 * h] + Rge[3 + i] * ld[3 * h + 1]) + Rge[6 + i] * ld[3 * h + 2];
}
// Step 4: the integrand from r.
__device__ __forceinline__ double joint_reaction_integrand(const GoalSet& GS, const mh_goal& G, const double* r) {
#pragma clang fp contract(off)
    const double* w6 = GS.gw + G.term_begin + 9;
    double L = 0.0;
    for (int i = 0; i < 6; ++i) L = L + w6[i] * (r[i] * r[i]);
    return L / w6[6];
}
// The workspace after the RNEA with the point's accelerations: the iterate's
// (implicit dynamics, one dae_eval), or the udot a first dae_eval solves, fed
// to a second one as prescribed accelerations (explicit dynamics).  One call
// site, so that the interpreter is inlined once.
template <class Z>
__device__ __forceinline__ void joint_reaction_dae(const DevModel& M, typename GenericDae<Z>::W& w, double t,
        const double* in) {
    double out[Z::MO], ud[Z::MQ];
    const int npass = M.implicit ? 1 : 2;
    for (int pass = 0; pass < npass; ++pass) {
        if (pass)
            for (int j = 0; j < Z::MQ; ++j) ud[j] = j < M.nq ? out[j] : 0.0;
        dae_eval<Z::MB, Z::MQ, Z::MP>(M, w, t, in, in + M.ns, out, pass ? ud : nullptr);
    }
}
// One thread per (grid point, lane) in the Lanes layout of k_eval (ND = NI -
// NSL + 2: the slack inputs stay as loaded and get no lane): L of every goal
// of kind 14, goal j of njr in goal order, to lv[(k stride + lane) njr + j].
// C (objective mode, base lanes only: stride 1): C[k ngoals + g] = quad[k] L.
// A lane carries the interpreter's whole workspace in scratch, as k_eval's.
template <class Z>
__global__ void __launch_bounds__(64) k_joint_reaction(DevModel M, Layout L, Lanes Ln, GoalSet GS, int njr,
        const double* __restrict__ x, const double* __restrict__ grid, const double* __restrict__ quad,
        double* __restrict__ C, double* __restrict__ lv) {
    using D = GenericDae<Z>;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)L.G * Ln.stride) return;
    const int k = (int)(gid / Ln.stride);
    const int r = (int)(gid - (long)k * Ln.stride);
    double in[D::MI];
    const double t = lane_inputs<D>(L, Ln, x, grid[k], k, r, in);
    typename D::W w;
    joint_reaction_dae<Z>(M, w, t, in);
    int j = 0;
    for (int g = 0; g < GS.ngoals; ++g) {
        const mh_goal G = GS.goals[g];
        if (G.kind != MH_GOAL_JOINT_REACTION) continue;
        double ld[6];
        joint_reaction_load(M, w, GS, G, ld);
        const double Lg = joint_reaction_integrand(GS, G, ld);
        if (j < njr) lv[(gid * njr) + j] = Lg;
        if (C) C[(long)k * GS.ngoals + g] = quad[k] * Lg;
        ++j;
    }
}
// The family's part of k_lane_goal_grad (goal_lanes.hpp): every direction is
// live for every goal, so every entry gets its sum added, a zero included.
struct JointReactionGoals : OneEntryPerGoal {
    static constexpr int kind = MH_GOAL_JOINT_REACTION;
    struct Args {};
    __device__ static bool live(const Args&, const GoalSet&, int, int) { return true; }
};
// mh_eval_joint_reaction: one thread per input row [time, NI point inputs],
// the six components of goal g's load.
template <class Z>
__global__ void __launch_bounds__(64) k_joint_reaction_probe(DevModel M, Layout L, GoalSet GS, int g, int npts,
        const double* __restrict__ in, double* __restrict__ outp) {
    using D = GenericDae<Z>;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = in + (long)p * (1 + L.NI);
    double v[D::MI];
#pragma unroll
    for (int i = 0; i < D::MI; ++i) v[i] = i < L.NI ? row[1 + i] : 0.0;
    typename D::W w;
    joint_reaction_dae<Z>(M, w, row[0], v);
    double ld[6];
    joint_reaction_load(M, w, GS, GS.goals[g], ld);
    for (int i = 0; i < 6; ++i) outp[(long)p * 6 + i] = ld[i];
}

template <class Z>
static void be_joint_reaction(mh_ctx* c, const double* x, int mode) {
    const LaneGoals& R = c->lane_goals[LG_JOINT_REACTION];
    launch_lane_goal_family<JointReactionGoals>(c, LG_JOINT_REACTION, {}, x, mode,
            [&](const Layout& L, const Lanes& ln, int mode) {
                // objective mode: c->g_block lanes per workgroup, as eval_g's k_eval
                const int tb = mode ? 64 : c->g_block;
                const long lanes = (long)c->G * ln.stride;
                hipLaunchKernelGGL(k_joint_reaction<Z>, dim3((unsigned)((lanes + tb - 1) / tb)), dim3(tb), 0,
                        c->stream, c->M, L, ln, c->GS, R.entries, x, c->d_grid, c->d_quad,
                        mode ? (double*)nullptr : c->d_C, R.lv);
            });
}
template <class Z>
static void be_joint_reaction_probe(mh_ctx* c, int goal, int np, const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    hipLaunchKernelGGL(k_joint_reaction_probe<Z>, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L, c->GS,
            goal, np, in, out);
}

const LaneGoalFamily& joint_reaction_goals() {
    static const LaneGoalFamily kFamily = {
        JointReactionGoals::kind,
        {&be_joint_reaction<SzSmall>, &be_joint_reaction<SzMedium>, &be_joint_reaction<SzLarge>,
         &be_joint_reaction<SzBody>}};
    return kFamily;
}
void joint_reaction_probe(mh_ctx* c, int goal, int np, const double* in, double* out) {
    static constexpr decltype(&be_joint_reaction_probe<SzSmall>) kProbe[4] = {
        &be_joint_reaction_probe<SzSmall>, &be_joint_reaction_probe<SzMedium>, &be_joint_reaction_probe<SzLarge>,
        &be_joint_reaction_probe<SzBody>};
    kProbe[c->size_class](c, goal, np, in, out);
}
