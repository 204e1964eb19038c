// accel_tracking.hip -- MocoAccelerationTrackingGoal's kernels (include/mocohip.h
// MH_GOAL_ACCELERATION_TRACKING): the linear acceleration in ground of a tracked
// frame's origin per finite-difference lane, from the lane's coordinates, speeds
// and accelerations.  The accelerations are the iterate's (implicit multibody
// dynamics: the kernel has no interpreter in it) or the udot of one run of the
// generic interpreter (explicit dynamics).  One instantiation per size class and
// dynamics mode, selected by the context's size class whatever back end serves
// g and J.  A translation unit of its own, as joint_reaction.hip:
// generic.hip compiles to the code it had without it.
#include "goal_lanes.hpp"

// One body of the forward kinematic pass of dae_eval (dae_device.hpp) with
// accelerations, restated: the parent's pose (Rp, pp), spatial velocity V and
// spatial acceleration A, all in ground about the ground origin, become body
// B's.  The base acceleration is zero (A = 0 at the ground: the interpreter's
// gravity-as-base-acceleration is not part of a kinematic acceleration).  The
// position part is joint_pose_stage's (mocohip.hip), statement for statement;
// the velocity and acceleration statements are steps 2a and 2b of the header,
// each operation rounded on its own.
template <class Q, class U, class UD>
__device__ __forceinline__ void accel_stage(const DevModel& M, const Q& q, const U& u, const UD& ud,
        const mh_body& B, double* Rp, double* pp, SV& V, SV& A) {
    double RGF[9], t0, t1, t2;
    mm3(Rp, B.R_PF, RGF);
    mv3(Rp, B.p_PF[0], B.p_PF[1], B.p_PF[2], t0, t1, t2);
    const double pGF0 = pp[0] + t0, pGF1 = pp[1] + t1, pGF2 = pp[2] + t2;
    const SV Vpar = V;
    double pFM0 = 0, pFM1 = 0, pFM2 = 0;
    for (int a = B.axis_begin; a < B.axis_begin + B.axis_count; ++a) {
        const mh_axis X = M.axes[a];
        if (X.type != MH_AXIS_TRANSLATION) continue;
        double v, d1, d2;
        fn_eval(M, X.func, q, v, d1, d2);
        pFM0 += v * X.dir[0]; pFM1 += v * X.dir[1]; pFM2 += v * X.dir[2];
        {
#pragma clang fp contract(off)
            const mh_function F = M.funcs[X.func];
            if (F.kind != MH_FN_CONSTANT) {   // step 2a: s = (0, R_GF dir), sd = Vpar x_m s
                const double s0 = (RGF[0] * X.dir[0] + RGF[1] * X.dir[1]) + RGF[2] * X.dir[2];
                const double s1 = (RGF[3] * X.dir[0] + RGF[4] * X.dir[1]) + RGF[5] * X.dir[2];
                const double s2 = (RGF[6] * X.dir[0] + RGF[7] * X.dir[1]) + RGF[8] * X.dir[2];
                const double e0 = Vpar.w1 * s2 - Vpar.w2 * s1, e1 = Vpar.w2 * s0 - Vpar.w0 * s2,
                             e2 = Vpar.w0 * s1 - Vpar.w1 * s0;
                const double uj = u[F.coord];
                const double thd = d1 * uj;
                const double thdd = (d2 * uj) * uj + d1 * ud[F.coord];
                V.v0 = V.v0 + s0 * thd; V.v1 = V.v1 + s1 * thd; V.v2 = V.v2 + s2 * thd;
                A.v0 = A.v0 + (e0 * thd + s0 * thdd);
                A.v1 = A.v1 + (e1 * thd + s1 * thdd);
                A.v2 = A.v2 + (e2 * thd + s2 * thdd);
            }
        }
    }
    mv3(RGF, pFM0, pFM1, pFM2, t0, t1, t2);
    const double oM0 = pGF0 + t0, oM1 = pGF1 + t1, oM2 = pGF2 + t2;
    double Rcur[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int a = B.axis_begin; a < B.axis_begin + B.axis_count; ++a) {
        const mh_axis X = M.axes[a];
        if (X.type != MH_AXIS_ROTATION) continue;
        double v, d1, d2;
        fn_eval(M, X.func, q, v, d1, d2);
        {
#pragma clang fp contract(off)
            const mh_function F = M.funcs[X.func];
            if (F.kind != MH_FN_CONSTANT) {   // step 2b: s = (w, oM x w), w = R_GF R_cur dir, sd = V x_m s
                double RGc[9];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j)
                        RGc[3 * i + j] = (RGF[3 * i] * Rcur[j] + RGF[3 * i + 1] * Rcur[3 + j]) +
                                         RGF[3 * i + 2] * Rcur[6 + j];
                const double w0 = (RGc[0] * X.dir[0] + RGc[1] * X.dir[1]) + RGc[2] * X.dir[2];
                const double w1 = (RGc[3] * X.dir[0] + RGc[4] * X.dir[1]) + RGc[5] * X.dir[2];
                const double w2 = (RGc[6] * X.dir[0] + RGc[7] * X.dir[1]) + RGc[8] * X.dir[2];
                const double s0 = oM1 * w2 - oM2 * w1, s1 = oM2 * w0 - oM0 * w2, s2 = oM0 * w1 - oM1 * w0;
                const double f0 = V.w1 * w2 - V.w2 * w1, f1 = V.w2 * w0 - V.w0 * w2, f2 = V.w0 * w1 - V.w1 * w0;
                const double e0 = (V.w1 * s2 - V.w2 * s1) + (V.v1 * w2 - V.v2 * w1);
                const double e1 = (V.w2 * s0 - V.w0 * s2) + (V.v2 * w0 - V.v0 * w2);
                const double e2 = (V.w0 * s1 - V.w1 * s0) + (V.v0 * w1 - V.v1 * w0);
                const double uj = u[F.coord];
                const double thd = d1 * uj;
                const double thdd = (d2 * uj) * uj + d1 * ud[F.coord];
                V.w0 = V.w0 + w0 * thd; V.w1 = V.w1 + w1 * thd; V.w2 = V.w2 + w2 * thd;
                V.v0 = V.v0 + s0 * thd; V.v1 = V.v1 + s1 * thd; V.v2 = V.v2 + s2 * thd;
                A.w0 = A.w0 + (f0 * thd + w0 * thdd);
                A.w1 = A.w1 + (f1 * thd + w1 * thdd);
                A.w2 = A.w2 + (f2 * thd + w2 * thdd);
                A.v0 = A.v0 + (e0 * thd + s0 * thdd);
                A.v1 = A.v1 + (e1 * thd + s1 * thdd);
                A.v2 = A.v2 + (e2 * thd + s2 * thdd);
            }
        }
        double Rk[9];
        axis_rot(X.dir[0], X.dir[1], X.dir[2], v, Rk);
        mm3(Rcur, Rk, Rcur);
    }
    double RGM[9];
    mm3(RGF, Rcur, RGM);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rp[3 * i + j] = RGM[3 * i] * B.R_BM[3 * j] + RGM[3 * i + 1] * B.R_BM[3 * j + 1] +
                            RGM[3 * i + 2] * B.R_BM[3 * j + 2];
    mv3(Rp, B.p_BM[0], B.p_BM[1], B.p_BM[2], t0, t1, t2);
    pp[0] = oM0 - t0; pp[1] = oM1 - t1; pp[2] = oM2 - t2;
}

// The linear acceleration in ground of the point at loc of body b (-1: ground,
// a = 0): b's ancestor chain walked root first with running pose, V and A and
// no per-body storage (the level-i ancestor is found by walking up from b),
// then step 3 of the header.
template <class Q, class U, class UD>
__device__ __forceinline__ void frame_acceleration(const DevModel& M, const Q& q, const U& u, const UD& ud, int b,
        const double* __restrict__ loc, double* acc) {
    double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pp[3] = {0, 0, 0};
    SV V = sv_zero(), A = sv_zero();
    int depth = 0;
    for (int x = b; x >= 0 && depth <= M.nb; x = M.bodies[x].parent) ++depth;
    for (int lev = depth - 1; lev >= 0; --lev) {
        int x = b;
        for (int i = 0; i < lev; ++i) x = M.bodies[x].parent;
        accel_stage(M, q, u, ud, M.bodies[x], Rp, pp, V, A);
    }
    {
#pragma clang fp contract(off)
        const double l0 = loc[0], l1 = loc[1], l2 = loc[2];
        const double r0 = pp[0] + ((Rp[0] * l0 + Rp[1] * l1) + Rp[2] * l2);
        const double r1 = pp[1] + ((Rp[3] * l0 + Rp[4] * l1) + Rp[5] * l2);
        const double r2 = pp[2] + ((Rp[6] * l0 + Rp[7] * l1) + Rp[8] * l2);
        // the point's velocity v + omega x r, then a0 + alpha x r + omega x (that)
        const double p0 = V.v0 + (V.w1 * r2 - V.w2 * r1), p1 = V.v1 + (V.w2 * r0 - V.w0 * r2),
                     p2 = V.v2 + (V.w0 * r1 - V.w1 * r0);
        acc[0] = (A.v0 + (A.w1 * r2 - A.w2 * r1)) + (V.w1 * p2 - V.w2 * p1);
        acc[1] = (A.v1 + (A.w2 * r0 - A.w0 * r2)) + (V.w2 * p0 - V.w0 * p2);
        acc[2] = (A.v2 + (A.w0 * r1 - A.w1 * r0)) + (V.w0 * p1 - V.w1 * p0);
    }
}

// Step 4: the integrand of goal G at time t.
template <class Q, class U, class UD>
__device__ __forceinline__ double accel_tracking_integrand(const DevModel& M, const GoalSet& GS, const mh_goal& G,
        double t, const Q& q, const U& u, const UD& ud) {
#pragma clang fp contract(off)
    double L = 0.0;
    for (int tb = G.term_begin; tb + 4 <= G.term_begin + G.term_count; tb += 4) {
        double a[3] = {0.0, 0.0, 0.0};
        const int b = GS.gidx[tb];
        if (b >= 0) frame_acceleration(M, q, u, ud, b, GS.gw + tb, a);
        const double d0 = a[0] - table_eval(M, G.table, GS.gcol[tb], t);
        const double d1 = a[1] - table_eval(M, G.table, GS.gcol[tb + 1], t);
        const double d2 = a[2] - table_eval(M, G.table, GS.gcol[tb + 2], t);
        L = L + GS.gw[tb + 3] * ((d0 * d0 + d1 * d1) + d2 * d2);
    }
    return L;
}

// Every goal of kind 15 at one lane: L of goal j of nat, in goal order, to
// lvl[j]; C (objective mode): C[g] = qk L.
template <class Q, class U, class UD>
__device__ __forceinline__ void accel_tracking_goals(const DevModel& M, const GoalSet& GS, int nat, double t,
        const Q& q, const U& u, const UD& ud, double qk, double* __restrict__ Ck, double* __restrict__ lvl) {
    int j = 0;
    for (int g = 0; g < GS.ngoals; ++g) {
        const mh_goal G = GS.goals[g];
        if (G.kind != MH_GOAL_ACCELERATION_TRACKING) continue;
        const double Lg = accel_tracking_integrand(M, GS, G, t, q, u, ud);
        if (j < nat) lvl[j] = Lg;
        if (Ck) Ck[g] = qk * Lg;
        ++j;
    }
}

// One thread per (grid point, lane) in the Lanes layout of k_eval (ND = NI -
// NSL + 2: the slack inputs get no lane): L of every goal of kind 15 to
// lv[(k stride + lane) nat + j].  live[d] (gradient mode; null: every lane):
// whether direction d can change L -- implicit dynamics: t0, tf and the
// coordinates, speeds and acceleration variables of the tracked chains; a lane
// of another direction is not evaluated and its quotient is not formed.
// C (objective mode, base lanes only: stride 1): C[k ngoals + g] = quad[k] L.
// EXPLICIT: udot = out[0..nq) of one dae_eval at the lane's inputs (one call
// site; the lane carries the interpreter's workspace in scratch, as k_eval's).
// Implicit: no interpreter; the inputs are read where they lie.
template <class Z, bool EXPLICIT>
__global__ void __launch_bounds__(64) k_accel_tracking(DevModel M, Layout L, Lanes Ln, GoalSet GS, int nat,
        const int* __restrict__ live, const double* __restrict__ x, const double* __restrict__ grid,
        const double* __restrict__ quad, double* __restrict__ C, double* __restrict__ lv) {
    using D = GenericDae<Z>;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)L.G * Ln.stride) return;
    const int k = (int)(gid / Ln.stride);
    const int r = (int)(gid - (long)k * Ln.stride);
    if (live && r != Ln.base && !live[r >= Ln.ND ? r - Ln.ND : r]) return;
    double* Ck = C ? C + (long)k * GS.ngoals : nullptr;
    const double qk = C ? quad[k] : 0.0;
    if constexpr (EXPLICIT) {
        double in[D::MI], out[D::MO];
        const double t = lane_inputs<D>(L, Ln, x, grid[k], k, r, in);
        typename D::W w;
        // (inlined here whatever the unit's other call sites suggest to the inliner: the workspace stays
        // private to the kernel and is reached with scratch instructions, not through a call)
        [[clang::always_inline]] dae_eval<Z::MB, Z::MQ, Z::MP>(M, w, t, in, in + M.ns, out, nullptr);
        accel_tracking_goals(M, GS, nat, t, in, in + M.nq, out, qk, Ck, lv + gid * nat);
    } else {
        PointIn in = point_in(L, x, k);
        const double t = lane_time(Ln, grid[k], x[0], x[1], r, in.pi, in.step);
        accel_tracking_goals(M, GS, nat, t, in, PointInAt{in, M.nq}, PointInAt{in, L.NS + L.NC}, qk, Ck,
                lv + gid * nat);
    }
}
// The family's part of k_lane_goal_grad (goal_lanes.hpp): liveness is per
// direction, the table k_accel_tracking skips lanes by, whatever the goal.
struct AccelTrackingGoals : OneEntryPerGoal {
    static constexpr int kind = MH_GOAL_ACCELERATION_TRACKING;
    struct Args {
        const int* __restrict__ live;
    };
    __device__ static bool live(const Args& A, const GoalSet&, int, int d) { return A.live[d]; }
};
// mh_eval_frame_accelerations: one thread per input row [time, NI point
// inputs], the acceleration of every frame of goal g, out[row][frame][3].
template <class Z, bool EXPLICIT>
__global__ void __launch_bounds__(64) k_accel_tracking_probe(DevModel M, Layout L, GoalSet GS, int g, int npts,
        const double* __restrict__ in, double* __restrict__ outp) {
    using D = GenericDae<Z>;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = in + (long)p * (1 + L.NI);
    const mh_goal G = GS.goals[g];
    const int nf = G.term_count / 4;
    double* o = outp + (long)p * nf * 3;
    if constexpr (EXPLICIT) {
        double v[D::MI], out[D::MO];
#pragma unroll
        for (int i = 0; i < D::MI; ++i) v[i] = i < L.NI ? row[1 + i] : 0.0;
        typename D::W w;
        [[clang::always_inline]] dae_eval<Z::MB, Z::MQ, Z::MP>(M, w, row[0], v, v + M.ns, out, nullptr);
        for (int f = 0; f < nf; ++f) {
            const int tb = G.term_begin + 4 * f, b = GS.gidx[tb];
            double a[3] = {0.0, 0.0, 0.0};
            if (b >= 0) frame_acceleration(M, v, v + M.nq, out, b, GS.gw + tb, a);
            for (int i = 0; i < 3; ++i) o[3 * f + i] = a[i];
        }
    } else {
        const PointIn v{row + 1, row + 1 + L.NS, row + 1 + L.NS + L.NC, L.NS, L.NC, -1, 0.0};
        for (int f = 0; f < nf; ++f) {
            const int tb = G.term_begin + 4 * f, b = GS.gidx[tb];
            double a[3] = {0.0, 0.0, 0.0};
            if (b >= 0) frame_acceleration(M, v, PointInAt{v, M.nq}, PointInAt{v, L.NS + L.NC}, b, GS.gw + tb, a);
            for (int i = 0; i < 3; ++i) o[3 * f + i] = a[i];
        }
    }
}

template <class Z, bool EXPLICIT>
static void launch_accel_tracking(mh_ctx* c, const double* x, int mode) {
    const LaneGoals& R = c->lane_goals[LG_ACCEL_TRACKING];
    launch_lane_goal_family<AccelTrackingGoals>(c, LG_ACCEL_TRACKING, {c->d_at_live}, x, mode,
            [&](const Layout& L, const Lanes& ln, int mode) {
                // objective mode: c->g_block lanes per workgroup, as eval_g's k_eval, and every lane live
                const int tb = mode ? 64 : c->g_block;
                const long lanes = (long)c->G * ln.stride;
                hipLaunchKernelGGL((k_accel_tracking<Z, EXPLICIT>), dim3((unsigned)((lanes + tb - 1) / tb)), dim3(tb),
                        0, c->stream, c->M, L, ln, c->GS, R.entries, mode ? c->d_at_live : (const int*)nullptr, x,
                        c->d_grid, c->d_quad, mode ? (double*)nullptr : c->d_C, R.lv);
            });
}
template <class Z>
static void be_accel_tracking(mh_ctx* c, const double* x, int mode) {
    if (c->M.implicit) launch_accel_tracking<Z, false>(c, x, mode);
    else launch_accel_tracking<Z, true>(c, x, mode);
}
template <class Z>
static void be_accel_tracking_probe(mh_ctx* c, int goal, int np, const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    if (c->M.implicit)
        hipLaunchKernelGGL((k_accel_tracking_probe<Z, false>), dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L,
                c->GS, goal, np, in, out);
    else
        hipLaunchKernelGGL((k_accel_tracking_probe<Z, true>), dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L,
                c->GS, goal, np, in, out);
}

const LaneGoalFamily& accel_tracking_goals() {
    static const LaneGoalFamily kFamily = {
        AccelTrackingGoals::kind,
        {&be_accel_tracking<SzSmall>, &be_accel_tracking<SzMedium>, &be_accel_tracking<SzLarge>,
         &be_accel_tracking<SzBody>}};
    return kFamily;
}
void accel_tracking_probe(mh_ctx* c, int goal, int np, const double* in, double* out) {
    static constexpr decltype(&be_accel_tracking_probe<SzSmall>) kProbe[4] = {
        &be_accel_tracking_probe<SzSmall>, &be_accel_tracking_probe<SzMedium>, &be_accel_tracking_probe<SzLarge>,
        &be_accel_tracking_probe<SzBody>};
    kProbe[c->size_class](c, goal, np, in, out);
}
