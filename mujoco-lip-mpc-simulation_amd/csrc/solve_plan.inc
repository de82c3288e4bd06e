// What one solve launches, in order, as data; and the row-step ladder of the compiled solve kernels.  Plain C++17 on
// standard headers alone (no HIP type, no handle, no environment), so that a host program can include this file by
// itself (tests/solve_plan_main.cpp).  launch_solve in host_api.inc issues the plan's steps in a flat loop;
// alipmpc_solve_launches counts its launches but the hand-off's, as it always has (ADVICE's open item, counting that
// one too, is the `kind != SP_HANDOFF` there).
//   ZERO_HEADER  a split launch's record counters are zeroed
//   ZERO_LIST    the stream's hand-off list is taken and its count zeroed (cfg.restoration = IPOPT on the lane program
//                and the fp32 wave program, which list the instances whose line search fails)
//   DD, LANE, SENS, SENS_OBS  that program's one launch (the sensitivity builds: resto = the restoration-capable one)
//   WAVE         the wave program in the handle's precision.  phase 0: the whole solve; 1: up to ckpt_it iterations or,
//                with team > 0, ckpt_tr line-search trials, then a record; 2: the records resume.  resto: the
//                restoration-capable build (fp64 alone; phase 1 runs the lean one).  form: QUEUE, the work queue over
//                the resident workgroups; ONE_WAVE, a wave per instance; TEAM, the team-capable build, `team` team
//                workgroups ahead of phase 2's single ones; PAIR, the paired phase 2.
//   HANDOFF      the listed instances, solved from their start by the fp64 restoration-capable work queue
// A batch splits when it has a cut (the trial cut counts in fp64 alone), 2 <= B <= slots, no launch order and a record
// buffer.  Without a split, B > slots of the build that runs takes the queue form.
#ifndef ALIPMPC_SOLVE_PLAN_INC
#define ALIPMPC_SOLVE_PLAN_INC

#include <algorithm>
#include <cstddef>
#include <type_traits>

namespace alip {

// ---- the row-step ladder: KSM = J-layout steps (4 rows each) of the compiled solve and sensitivity kernels
constexpr int KSM_LADDER[] = {4, 8, 10, 12, 16, 24, 32, 48};
constexpr int KSM_NONE = 1 << 20;   // no compiled size covers the rows (alipmpc_create refuses the handle)

// the smallest compiled KSM covering `rows` rows; mo4 is rounded up to 4 * ksm_of(rows)
inline int ksm_of(int rows)
{
    for (int k : KSM_LADDER)
        if (rows <= 4 * k) return k;
    return KSM_NONE;
}

// f(std::integral_constant<int, KSM>) for the compiled size covering mo4 rows (the largest one beyond the ladder)
template <std::size_t I = 0, class F>
void with_ksm(int mo4, F&& f)
{
    constexpr int K = KSM_LADDER[I];
    if constexpr (I + 1 == sizeof(KSM_LADDER) / sizeof(KSM_LADDER[0]))
        f(std::integral_constant<int, K>{});
    else if (mo4 <= 4 * K)
        f(std::integral_constant<int, K>{});
    else
        with_ksm<I + 1>(mo4, f);
}

// ---- the plan
constexpr long long SP_TEAM_CAP = 128;   // team workgroups of a phase-2 launch (alip::TEAM_CAP)

enum SpProgram { SP_PROG_DD, SP_PROG_LANE, SP_PROG_WAVE_F64, SP_PROG_WAVE_F32, SP_PROG_SENS, SP_PROG_SENS_OBS };
enum SpKind { SP_ZERO_HEADER, SP_ZERO_LIST, SP_DD, SP_LANE, SP_SENS, SP_SENS_OBS, SP_WAVE, SP_HANDOFF };
enum SpForm { SP_QUEUE, SP_ONE_WAVE, SP_TEAM, SP_PAIR };

struct SpFacts {
    SpProgram program;
    bool resto_ipopt;         // cfg.restoration = IPOPT on a LIP variant (KP.resto_ipopt)
    long long B;
    long long slots;          // instances resident at once on the lean work-queue build (alipmpc_solve_slots)
    long long slots_resto;    // and on the fp64 restoration-capable one (read for a one-phase launch of that build)
    int split_it, split_tr;   // the cuts (0 = off)
    bool split_pair;          // the handle has the paired phase 2 (set on fp64 restoration handles alone)
    bool allow_pair;          // and the caller takes it (the batch API; the closed loop keeps the 4-wave form)
    bool ordered;             // the batch has a launch order (KP.order)
    bool records;             // the stream has a record buffer
};

struct SpStep {
    SpKind kind;
    int phase;
    bool resto;
    SpForm form;
    int team, ckpt_it, ckpt_tr;
};

struct SpPlan {   // (fixed capacity: the longest plan is the fp32 split with its hand-off)
    int n = 0;
    SpStep step[5];
    const SpStep* begin() const { return step; }
    const SpStep* end() const { return step + n; }
    void add(SpKind kind, int phase = 0, bool resto = false, SpForm form = SP_QUEUE, int team = 0, int it = 0, int tr = 0)
    {
        step[n++] = SpStep{kind, phase, resto, form, team, it, tr};
    }
};

inline bool sp_is_launch(SpKind k) { return k != SP_ZERO_HEADER && k != SP_ZERO_LIST; }

// the trial cut as the program takes it
inline int sp_trial_cut(const SpFacts& f) { return f.program == SP_PROG_WAVE_F64 ? f.split_tr : 0; }

// whether the batch splits once its stream has a record buffer (the driver asks before it looks for one)
inline bool sp_splits(const SpFacts& f)
{
    const bool wave = f.program == SP_PROG_WAVE_F64 || f.program == SP_PROG_WAVE_F32;
    return wave && (f.split_it > 0 || sp_trial_cut(f) > 0) && f.B >= 2 && f.B <= f.slots && !f.ordered;
}

inline SpPlan solve_plan(const SpFacts& f)
{
    SpPlan p;
    switch (f.program) {
    case SP_PROG_DD:
        p.add(SP_DD);
        return p;
    case SP_PROG_SENS:
    case SP_PROG_SENS_OBS:
        p.add(f.program == SP_PROG_SENS ? SP_SENS : SP_SENS_OBS, 0, f.resto_ipopt);
        return p;
    case SP_PROG_LANE:
        if (f.resto_ipopt) p.add(SP_ZERO_LIST);
        p.add(SP_LANE);
        if (f.resto_ipopt) p.add(SP_HANDOFF, 0, true);
        return p;
    default:
        break;
    }
    const bool resto = f.resto_ipopt && f.program == SP_PROG_WAVE_F64;      // the build with the restoration phase
    const bool handoff = f.resto_ipopt && f.program == SP_PROG_WAVE_F32;    // (fp32 has the lean build only)
    const bool split = sp_splits(f) && f.records;
    if (split) p.add(SP_ZERO_HEADER);
    if (handoff) p.add(SP_ZERO_LIST);
    if (!split) {
        p.add(SP_WAVE, 0, resto, f.B > (resto ? f.slots_resto : f.slots) ? SP_QUEUE : SP_ONE_WAVE);
    } else {
        const int tr = sp_trial_cut(f);
        const int team = tr > 0 ? (int)std::min(f.B, SP_TEAM_CAP) : 0;
        const SpForm form = team > 0 ? SP_TEAM : SP_ONE_WAVE;
        p.add(SP_WAVE, 1, false, form, team, std::max(f.split_it, 0), tr);
        p.add(SP_WAVE, 2, resto, f.allow_pair && f.split_pair && team == 0 && resto ? SP_PAIR : form, team);
    }
    if (handoff) p.add(SP_HANDOFF, 0, true);
    return p;
}

}  // namespace alip

#endif  // ALIPMPC_SOLVE_PLAN_INC
