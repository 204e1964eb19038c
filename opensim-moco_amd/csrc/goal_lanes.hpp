// goal_lanes.hpp -- what the goals evaluated on finite-difference lanes share
// (joint_reaction.hip, accel_tracking.hip, muscle_outputs.hip, metabolics.hip):
// a lane's inputs read where they lie, the gradient kernel over a family's lane
// values, and the launch of a family's kernels in objective or gradient mode.
// Each family keeps its lane kernel, in a translation unit of its own.
#pragma once
#include "core.hpp"

// The point inputs of one grid point where they lie (x, or a probe row) with a
// lane's perturbation applied on the fly, lane_inputs' arithmetic (in[i] + step)
// with nothing staged per thread: states, controls and derivative variables.
struct PointIn {
    const double* __restrict__ xs;
    const double* __restrict__ xc;
    const double* __restrict__ xd;
    int NS, NC, pi;
    double step;
    __device__ __forceinline__ double operator[](int i) const {
#pragma clang fp contract(off)
        const double v = i < NS ? xs[i] : (i < NS + NC ? xc[i - NS] : xd[i - NS - NC]);
        return i == pi ? v + step : v;
    }
};
// Inputs o, o + 1, ... of a PointIn: the speeds (o = nq) and the derivative
// variables (o = NS + NC).
struct PointInAt {
    const PointIn& in;
    int o;
    __device__ __forceinline__ double operator[](int j) const { return in[o + j]; }
};
// Grid point k of the iterate x, unperturbed (lane_time sets pi and step).
__device__ __forceinline__ PointIn point_in(const Layout& L, const double* __restrict__ x, int k) {
    return PointIn{x + 2 + (long)k * L.NS, x + 2 + (long)L.NS * L.G + (long)k * L.NC, x + L.DB + (long)k * L.NDV,
                   L.NS, L.NC, -1, 0.0};
}

// Where direction d (0 = t0, 1 = tf, 2 + i = point input i: states, controls,
// derivative variables, multipliers) of grid point k lands: the point's part
// of the t0 / tf derivative, or the input's entry of the gradient.
__device__ __forceinline__ double* grad_entry(const Layout& L, double* __restrict__ tpart,
        double* __restrict__ grad, int k, int d) {
    if (d < 2) return tpart + ((long)k * 2 + d);
    const int i = d - 2;
    if (i < L.NS) return grad + (2 + (long)k * L.NS + i);
    if (i < L.NS + L.NC) return grad + (2 + (long)L.NS * L.G + (long)k * L.NC + (i - L.NS));
    if (i < L.NS + L.NC + L.NDV) return grad + (L.DB + (long)k * L.NDV + (i - L.NS - L.NC));
    return grad + (L.XM + (long)k * L.NM + (i - L.NS - L.NC - L.NDV));
}

// The gradient kernel of every lane-goal family, one thread per (grid point,
// direction).  lv holds the family's lane values [G][stride][nent] in the
// Lanes layout of k_eval, a goal's entries side by side in goal order.  The
// quotients are k_grad's formulas and arithmetic; G.weight * dur * quad[k] *
// dL of the goals the direction is live for, summed in goal order, is added to
// what the kernels before it on the stream left in grad / tpart (k_grad,
// k_marker_tracking, then the families in launch_lane_goals' order: one writer
// per entry and launch).  Direction 0 also writes the goals' integrand slots
// of C.  A direction live for no goal writes nothing: its entry keeps its bits.
// A family's policy P gives
//   kind                          the goals' kind
//   Args                          what its functions read besides the goals
//   entries(G)                    the lane values goal G occupies
//   live(A, GS, g, d)             whether direction d can change goal g
//   value(A, GS, Ln, g, lk, nent, e, r)
//                                 goal g (first entry e) at lane r of the
//                                 point's lane block lk
template <class P>
__global__ void __launch_bounds__(64) k_lane_goal_grad(typename P::Args A, Layout L, Lanes Ln, GoalSet GS,
        int nent, const double* __restrict__ x, const double* __restrict__ quad, const double* __restrict__ lv,
        double* __restrict__ C, double* __restrict__ grad, double* __restrict__ tpart) {
#pragma clang fp contract(off)
    const int ND = Ln.ND;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)L.G * ND) return;
    const int k = (int)(tid / ND), d = (int)(tid % ND);
    const double dur = x[1] - x[0], h = Ln.h;
    const double* lk = lv + (long)k * Ln.stride * nent;
    double acc = 0.0;
    bool any = false;
    int e = 0;
    for (int g = 0; g < GS.ngoals && e < nent; ++g) {
        const mh_goal G = GS.goals[g];
        if (G.kind != P::kind) continue;
        if (P::live(A, GS, g, d)) {
            const double l1 = P::value(A, GS, Ln, g, lk, nent, e, d);
            double dL;
            if (Ln.fd == MH_FD_CENTRAL) {
                dL = (l1 - P::value(A, GS, Ln, g, lk, nent, e, ND + d)) / (2.0 * h);
            } else {
                const double l0 = P::value(A, GS, Ln, g, lk, nent, e, Ln.base);
                dL = Ln.fd == MH_FD_FORWARD ? (l1 - l0) / h : (l0 - l1) / h;
            }
            acc += G.weight * dur * quad[k] * dL;
            any = true;
            if (d == 0) C[(long)k * GS.ngoals + g] = quad[k] * P::value(A, GS, Ln, g, lk, nent, e, Ln.base);
        }
        e += P::entries(G);
    }
    if (any) *grad_entry(L, tpart, grad, k, d) += acc;
}

// The policy parts of a family whose goals occupy one lane value each.
struct OneEntryPerGoal {
    __device__ static int entries(const mh_goal&) { return 1; }
    template <class Args>
    __device__ static double value(const Args&, const GoalSet&, const Lanes&, int, const double* __restrict__ lk,
            int nent, int e, int r) {
        return lk[(long)r * nent + e];
    }
};

// A family's kernels in objective mode (mode 0: base lanes only, a stride of
// one) or gradient mode (mode 1: every lane, then k_lane_goal_grad<P>).
// lanes(L, ln, mode) launches the family's lane kernel: its grid shape and
// arguments are the family's own.
template <class P, class F>
static void launch_lane_goal_family(mh_ctx* c, int family, const typename P::Args& A, const double* x, int mode,
        const F& lanes) {
    const Layout L = make_layout(c, 0, c->G);
    const LaneGoals& R = c->lane_goals[family];
    if (mode == 0) {
        lanes(L, Lanes{c->fd, c->goal_lanes.ND, 1, 0, c->h}, 0);
        return;
    }
    const Lanes& ln = c->goal_lanes;
    lanes(L, ln, 1);
    const long dirs = (long)c->G * ln.ND;
    hipLaunchKernelGGL(k_lane_goal_grad<P>, dim3((unsigned)((dirs + 63) / 64)), dim3(64), 0, c->stream, A, L, ln,
            c->GS, R.entries, x, c->d_quad, R.lv, c->d_C, c->d_grad, c->d_tpart);
}
