// The closed loop's tick plan: which launches a call issues, in order, as data.  Plain C++17 on standard headers alone
// (no HIP type, no handle, no environment), so that a host program can include this file by itself
// (tests/cl_ticks_main.cpp); closed_loop_host.inc issues the plan's segments, group by group.
//
// Tick t = s * f_cyc + i is tick i of step s.  A scheduled loop solves on the ticks whose bit of the mask is set, an
// unscheduled one on every tick.  mode is cfg.cl_between: 0 runs nominal ticks between the solves; 1 (first order) has
// a solve leave anchors when a later tick of its step does not solve, and the step is then live until its end or
// until a solve of it leaves none; 3 (guarded) is mode 1 with every non-solve tick of a live step taken one at a time.
//   SOLVE        one tick.  anchor: modes 1 and 3, a later tick of the step does not solve (the sensitivity build runs in
//                the solve's place and leaves anchors).  live: the step was live before this tick.
//   NOMINAL_RUN  nt >= 1 consecutive non-solve ticks from t0: one launch.  fuse extends a run while the next tick does
//                not solve: a live run to the end of its step, any other across step boundaries up to S * f_cyc;
//                without fuse every run is one tick.  live: the anchored episodes run the first-order kernel.
//   GUARDED      mode 3 alone: one non-solve tick of a live step.  anchor: as for a solve of this tick index.
#ifndef ALIPMPC_CL_TICKS_INC
#define ALIPMPC_CL_TICKS_INC

#include <cstdint>
#include <vector>

constexpr int CL_MODE_FIRST_ORDER = 1, CL_MODE_GUARDED = 3;   // cfg.cl_between (alipmpc.h)

enum ClTickKind { CL_SOLVE, CL_NOMINAL_RUN, CL_GUARDED };

struct ClSeg {
    ClTickKind kind;
    long long t0;   // first tick, s * f_cyc + i
    int nt;         // ticks (1 unless NOMINAL_RUN)
    int s, i;       // step and tick index of t0
    bool live, anchor;
};

inline std::vector<ClSeg> cl_tick_plan(int S, int f_cyc, bool scheduled, uint64_t mask, int mode, bool fuse)
{
    const bool guarded = scheduled && mode == CL_MODE_GUARDED;
    const bool first_order = (scheduled && mode == CL_MODE_FIRST_ORDER) || guarded;
    auto solves = [&](int i) { return !scheduled || ((mask >> i) & 1ull) != 0; };
    // does a tick of the step after tick i not solve
    auto anchors = [&](int i) {
        for (int j = i + 1; j < f_cyc; ++j)
            if (!solves(j)) return true;
        return false;
    };
    std::vector<ClSeg> plan;
    int live_step = -1;   // the step in which a solve tick last left anchors
    const long long TT = (long long)S * f_cyc;
    for (long long t = 0; t < TT;) {
        const int s = (int)(t / f_cyc), i = (int)(t % f_cyc);
        const bool live = live_step == s;
        if (solves(i)) {
            const bool anchor = first_order && anchors(i);
            plan.push_back({CL_SOLVE, t, 1, s, i, live, anchor});
            live_step = anchor ? s : -1;
            ++t;
        } else if (guarded && live) {
            plan.push_back({CL_GUARDED, t, 1, s, i, true, anchors(i)});
            ++t;
        } else {
            const long long tend = live ? (long long)(s + 1) * f_cyc : TT;
            long long t1 = t + 1;
            while (fuse && t1 < tend && !solves((int)(t1 % f_cyc))) ++t1;
            plan.push_back({CL_NOMINAL_RUN, t, (int)(t1 - t), s, i, live, false});
            t = t1;
        }
    }
    return plan;
}

#endif  // ALIPMPC_CL_TICKS_INC
