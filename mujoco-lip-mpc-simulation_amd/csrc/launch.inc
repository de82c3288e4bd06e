// ------------------------------------------------------------------------------------------------
// kernel launchers (included by alipmpc.hip into every translation unit, inside namespace alip).  The library may be
// built as one translation unit per horizon N (ALIP_PART = N: that horizon's kernels and the launchers templated on N,
// which are declared in every part and explicitly instantiated in part N), ALIP_PART = 7 / 8 (the lane solver, fp64 /
// fp32, and launch_lane<R>) plus ALIP_PART = 0 (host code, C ABI, rollout kernels), compiled in parallel and linked
// into one .so; without ALIP_PART everything is one TU.
// A launcher launches what it is told (solve_plan.inc decides which build and form a solve runs); each rule of this
// layer is written once: with_n (a run-time horizon as a compile-time N), with_ksm (solve_plan.inc: the row-step
// ladder), capped_grid, wave_kernel (the solve kernel of a build and form).
// ------------------------------------------------------------------------------------------------
using Kern = void (*)(KP);

// f(std::integral_constant<int, N>) for the horizon N = 1 .. ALIPMPC_MAX_N; `none` for any other
template <class F, class T>
T with_n(int N, T none, F&& f)
{
    switch (N) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    }
    return none;
}
static_assert(ALIPMPC_MAX_N == 6, "with_n covers every horizon");

// dynamic-LDS opt-in, once per kernel and size (hipFuncSetAttribute is a host round trip: keep it out of the
// steady-state launch path)
static void set_smem(const void* f, size_t smem)
{
    static std::mutex mtx;
    static std::unordered_map<const void*, size_t> done[64];   // per device ordinal
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mtx);
    auto& d = done[dev & 63];
    auto it = d.find(f);
    if (it != d.end() && it->second >= smem) return;
    // (r5a: at N = 6 this call failed for a kernel variant that was not launched — its workgroup's LDS above the CU's
    // 160 KB — and the error it left was picked up by the launch's hipGetLastError, so every N = 6 solve reported
    // "invalid argument".  A failure is consumed here; launching a kernel whose LDS does not fit fails on its own.)
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    d[f] = smem;
}

// workgroups of kernel f resident on the whole device at once (occupancy x CUs), cached per (f, smem)
static unsigned resident_blocks(const void* f, size_t smem, int threads = WAVE * WAVES_PER_BLOCK)
{
    static std::mutex mtx;
    static std::map<std::pair<const void*, size_t>, unsigned> cache[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mtx);
    auto& c = cache[dev & 63];
    auto it = c.find({f, smem});
    if (it != c.end()) return it->second;
    int per_cu = 0, cus = 0;
    unsigned r = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, smem) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu > 0 && cus > 0)
        r = (unsigned)per_cu * (unsigned)cus;
    c[{f, smem}] = r;
    return r;
}

// the grid of a grid-stride or work-queue kernel: a workgroup per `need` units of work, at most the resident ones
// (res = 0, occupancy unknown: uncapped), at least one
inline unsigned capped_grid(unsigned res, unsigned need) { return res > 0 && res < need ? res : (need > 0 ? need : 1u); }
inline unsigned groups_of(long long B, long long per) { return (unsigned)((B + per - 1) / per); }

// the team-capable build's workgroup LDS: smem (KP, G and WAVES_PER_BLOCK workspaces) with TEAM_WAVES workspaces
template <int N, class R>
size_t team_smem(size_t smem)
{
    const size_t fixed = sizeof(double) * (size_t)KP_DOUBLES + sizeof(R) * (size_t)Dim<N>::NG * Dim<N>::NCP;
    return fixed + (smem - fixed) / WAVES_PER_BLOCK * TEAM_WAVES;
}

// the paired phase-2 build's workgroup LDS: PAIR_WAVES workspaces (fp64)
template <int N>
size_t pair_smem(size_t smem)
{
    const size_t fixed = sizeof(double) * ((size_t)KP_DOUBLES + (size_t)Dim<N>::NG * Dim<N>::NCP);
    return fixed + (smem - fixed) / WAVES_PER_BLOCK * PAIR_WAVES;
}
// (compiled for the shapes with one row group per lane, the 2-waves-per-SIMD restoration-capable builds)
constexpr bool pair_ksm(int ksm) { return 4 * ksm <= WAVE; }

// ---- the launchers templated on the horizon: declared in every part, defined in their own
// the wave program's solve kernels in precision f32 / fp64: the resident workgroups of the work-queue build (resto: the
// restoration-capable one), and one launch of the given build in the given form (smem: smem_bytes of that precision)
template <int N>
unsigned wave_resident(bool f32, bool resto, int mo4, size_t smem);
template <int N>
hipError_t launch_wave(bool f32, bool resto, SpForm form, const KP& P, size_t smem, hipStream_t st);
template <int N>
hipError_t launch_sens(bool obs, bool resto, const KP& P, size_t smem, hipStream_t st);
template <int N>
hipError_t launch_eval(const KP& P, size_t smem, hipStream_t st);
template <int N>
hipError_t launch_dd(bool solve, const KP& P, size_t smem, hipStream_t st);

#if !defined(ALIP_PART) || (ALIP_PART >= 1 && ALIP_PART <= ALIPMPC_MAX_N)
// the solve kernel of a build and form; nullptr where none is compiled.  The team-capable build exists in fp64 only: in
// fp32 its different code rounded differently from the plain build's (fp32 contraction / packing decisions depend on
// the surrounding code), so fp32 splits never make team records; fp32 has the lean build only (a failed search hands
// the instance to the fp64 wave program).
template <int N, int K, class R>
Kern wave_kernel(bool resto, SpForm form)
{
    if constexpr (sizeof(R) == 8) {
        if (resto) {
            if constexpr (pair_ksm(K))
                if (form == SP_PAIR) return solve_kernel<N, K, R, true, false, true, true>;
            return form == SP_QUEUE ? solve_kernel<N, K, R, false, false, true>
                 : form == SP_ONE_WAVE ? solve_kernel<N, K, R, true, false, true>
                 : form == SP_TEAM ? solve_kernel<N, K, R, true, true, true> : nullptr;
        }
        return form == SP_QUEUE ? solve_kernel<N, K, R, false> : form == SP_ONE_WAVE ? solve_kernel<N, K, R, true>
             : form == SP_TEAM ? solve_kernel<N, K, R, true, true> : nullptr;
    } else {
        return form == SP_QUEUE ? solve_kernel<N, K, R, false> : form == SP_ONE_WAVE ? solve_kernel<N, K, R, true> : nullptr;
    }
}

template <int N, int K, class R>
unsigned wave_resident_k(bool resto, size_t smem)
{
    const Kern kq = wave_kernel<N, K, R>(resto, SP_QUEUE);
    set_smem((const void*)kq, smem);
    return resident_blocks((const void*)kq, smem);
}

template <int N, int K, class R>
hipError_t launch_wave_k(bool resto, SpForm form, const KP& P, size_t smem, hipStream_t st)
{
    const Kern kern = wave_kernel<N, K, R>(resto, form);
    if (!kern) return hipErrorInvalidValue;
    if (form == SP_PAIR) {
        // the paired phase 2 (alipmpc_create checked that its workgroup fits the LDS): the worst-case grid —
        // ceil(np / 4) workgroups with pending records, then 8 regular records each, np + nr <= B
        const size_t smem_p = pair_smem<N>(smem);
        set_smem((const void*)kern, smem_p);
        hipLaunchKernelGGL(kern, dim3(groups_of(P.B, 4) + 1u), dim3(WAVE * PAIR_WAVES), smem_p, st, P);
        return hipGetLastError();
    }
    // the opt-in of the build's queue, one-wave and team kernels, whichever runs now: a later launch in another form
    // (inside a stream capture perhaps) finds it made.  The team-capable build (fp64; in fp32 its place is the one-wave
    // kernel's) runs only where its workgroup fits the LDS: alipmpc_create clears the trial cuts otherwise
    const size_t smem_t = team_smem<N, R>(smem);
    const Kern k1 = wave_kernel<N, K, R>(resto, SP_ONE_WAVE);
    set_smem((const void*)wave_kernel<N, K, R>(resto, SP_QUEUE), smem);
    set_smem((const void*)k1, smem);
    if (smem_t <= 160 * 1024) set_smem(sizeof(R) == 8 ? (const void*)wave_kernel<N, K, R>(resto, SP_TEAM) : (const void*)k1, smem_t);
    const unsigned res = form == SP_QUEUE ? resident_blocks((const void*)kern, smem) : 0u;
    if (res > 0)                 // the persistent work queue over the resident workgroups
        hipLaunchKernelGGL(kern, dim3(res), dim3(WAVE * WAVES_PER_BLOCK), smem, st, P);
    else if (form == SP_TEAM)    // team records: phase 2 has P.team team workgroups ahead of the one-wave-per-instance ones
        hipLaunchKernelGGL(kern, dim3(capped_grid(0, (P.resume ? (unsigned)P.team : 0u) + groups_of(P.B, TEAM_WAVES))),
                           dim3(WAVE * TEAM_WAVES), smem_t, st, P);
    else                         // one instance per wave (and a queue launch whose occupancy is unknown)
        hipLaunchKernelGGL(k1, dim3(capped_grid(0, groups_of(P.B, WAVES_PER_BLOCK))), dim3(WAVE * WAVES_PER_BLOCK), smem, st, P);
    return hipGetLastError();
}

// dev builds for register reports (tools/regs.py, ALIP_DEV_ONLY_KSM) compile the solve kernels of one row-step count,
// fp64 only; the sensitivity builds keep the ladder
template <class F>
void with_wave_ksm(int mo4, F&& f)
{
#ifdef ALIP_DEV_ONLY_KSM
    (void)mo4;
    f(std::integral_constant<int, ALIP_DEV_ONLY_KSM>{});
#else
    with_ksm(mo4, f);
#endif
}
#ifdef ALIP_DEV_ONLY_KSM
constexpr bool WAVE_F32 = false;
#else
constexpr bool WAVE_F32 = true;
#endif

template <int N>
unsigned wave_resident(bool f32, bool resto, int mo4, size_t smem)
{
    unsigned res = 0;
    with_wave_ksm(mo4, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if constexpr (WAVE_F32)
            if (f32) {
                res = wave_resident_k<N, K, float>(resto, smem);
                return;
            }
        res = wave_resident_k<N, K, double>(resto, smem);
    });
    return res;
}

template <int N>
hipError_t launch_wave(bool f32, bool resto, SpForm form, const KP& P, size_t smem, hipStream_t st)
{
    hipError_t e = hipSuccess;
    with_wave_ksm(P.mo4, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if constexpr (WAVE_F32)
            if (f32) {
                e = launch_wave_k<N, K, float>(resto, form, P, smem, st);
                return;
            }
        e = launch_wave_k<N, K, double>(resto, form, P, smem, st);
    });
    return e;
}

// the sensitivity build (fp64, N <= 5: n <= 15, the gj_regs domain): the persistent work queue over at most the
// resident workgroups, whatever B is
template <int N>
hipError_t launch_sens(bool obs, bool resto, const KP& P, size_t smem, hipStream_t st)
{
    if constexpr (Dim<N>::n > ALIP_GJ_MAX_N || Dim<N>::n > 15) {
        return hipErrorNotSupported;
    } else {
        with_ksm(P.mo4, [&](auto k) {
            constexpr int K = decltype(k)::value;
            const Kern kq = obs ? (resto ? sens_obs_kernel<N, K, true> : sens_obs_kernel<N, K, false>)
                                : (resto ? sens_kernel<N, K, true> : sens_kernel<N, K, false>);
            set_smem((const void*)kq, smem);
            const unsigned grid = capped_grid(resident_blocks((const void*)kq, smem), groups_of(P.B, WAVES_PER_BLOCK));
            hipLaunchKernelGGL(kq, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), smem, st, P);
        });
        return hipGetLastError();
    }
}

// the eval hook, always fp64: the grid-stride eval kernel (16 instances per workgroup)
template <int N>
hipError_t launch_eval(const KP& P, size_t smem, hipStream_t st)
{
    set_smem((const void*)eval_kernel<N>, smem);
    const unsigned grid = capped_grid(resident_blocks((const void*)eval_kernel<N>, smem), groups_of(P.B, GROUPS_PER_BLOCK));
    hipLaunchKernelGGL(eval_kernel<N>, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), smem, st, P);
    return hipGetLastError();
}

template <int N>
hipError_t launch_dd(bool solve, const KP& P, size_t smem, hipStream_t st)
{
    const Kern kern = !solve ? dd_eval_kernel<N>
                      : P.mo4 <= WAVE ? dd_solve_kernel<N, 1> : P.mo4 <= 2 * WAVE ? dd_solve_kernel<N, 2> : dd_solve_kernel<N, 3>;
    set_smem((const void*)kern, smem);
    hipLaunchKernelGGL(kern, dim3(groups_of(P.B, WAVES_PER_BLOCK)), dim3(WAVE * WAVES_PER_BLOCK), smem, st, P);
    return hipGetLastError();
}

#ifdef ALIP_PART
template unsigned wave_resident<ALIP_PART>(bool, bool, int, size_t);
template hipError_t launch_wave<ALIP_PART>(bool, bool, SpForm, const KP&, size_t, hipStream_t);
template hipError_t launch_sens<ALIP_PART>(bool, bool, const KP&, size_t, hipStream_t);
template hipError_t launch_eval<ALIP_PART>(const KP&, size_t, hipStream_t);
template hipError_t launch_dd<ALIP_PART>(bool, const KP&, size_t, hipStream_t);
#endif
#endif

// lane solver (lane_solve.inc): N = 3, NC = compiled circle slots (>= cfg.nc_max), or (nct = LANE_FORM5, modi) the
// form build's 5 obstacle-form slots (circles and ellipses, >= cfg.nc_max + cfg.ne_max).  A persistent
// grid of at most the resident one-wave workgroups; each lane takes instances from the launch's work queue.
constexpr int LANE_FORM5 = 100 + 5;
template <class R>
unsigned lane_resident(int nct, bool modi);   // (0: no such build)
template <class R>
hipError_t launch_lane(int nct, bool modi, const KP& P, hipStream_t st);

#if !defined(ALIP_PART) || ALIP_PART == 7 || ALIP_PART == 8
template <class R>
Kern lane_kernel_of(int nct, bool modi)
{
    if (modi)
        return nct == 0 ? lane_kernel<3, 0, true, R> : nct == 5 ? lane_kernel<3, 5, true, R>
             : nct == 6 ? lane_kernel<3, 6, true, R>
             : nct == LANE_FORM5 ? lane_kernel<3, 5, true, lane::Form<R>> : nullptr;
    return nct == 0 ? lane_kernel<3, 0, false, R> : nct == 5 ? lane_kernel<3, 5, false, R>
         : nct == 6 ? lane_kernel<3, 6, false, R> : nullptr;
}
template <class R>
unsigned lane_resident(int nct, bool modi)
{
    const Kern kern = lane_kernel_of<R>(nct, modi);
    return kern ? resident_blocks((const void*)kern, 0, WAVE) : 0u;
}
template <class R>
hipError_t launch_lane(int nct, bool modi, const KP& P, hipStream_t st)
{
    const Kern kern = lane_kernel_of<R>(nct, modi);
    if (!kern) return hipErrorInvalidValue;
    // not capped by the work: small batches are spread over every resident wave (the kernel's first fetch takes
    // ceil(B / grid))
    const unsigned res = lane_resident<R>(nct, modi);
    hipLaunchKernelGGL(kern, dim3(res > 0 ? res : capped_grid(0, groups_of(P.B, WAVE))), dim3(WAVE), 0, st, P);
    return hipGetLastError();
}
#if defined(ALIP_PART) && ALIP_PART == 7
template unsigned lane_resident<double>(int, bool);
template hipError_t launch_lane<double>(int, bool, const KP&, hipStream_t);
#elif defined(ALIP_PART)
template unsigned lane_resident<float>(int, bool);
template hipError_t launch_lane<float>(int, bool, const KP&, hipStream_t);
#endif
#endif

// sweep kernel (eval hook, N = 3, circles only): CH-instance chunks per wave, WPG waves per workgroup, a grid-stride
// over the chunks on at most the resident workgroups
hipError_t launch_sweep(int nc, bool fen, const KP& P, hipStream_t st);
#if ALIP_PART_N(3)
template <int NC, bool FEN, int CH, int WPG>
void launch_sweep_t(const KP& P, hipStream_t st)
{
    using L = SweepL<NC, FEN>;
    auto kern = sweep_kernel<NC, FEN, CH, WPG>;
    const size_t smem = sizeof(double) * ((size_t)L::GL + (size_t)WPG * (CH / 2) * L::SLOTD);
    set_smem((const void*)kern, smem);
    const unsigned grid = capped_grid(resident_blocks((const void*)kern, smem, WAVE * WPG), groups_of(P.B, (long long)CH * WPG));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVE * WPG), smem, st, P);
}
template <int NC, bool FEN>
void launch_sweep_s(const KP& P, hipStream_t st)
{
    // instances per wave x waves per workgroup (LDS: the G/E copy per workgroup + CH/2 coefficient slots per
    // wave); ALIPMPC_SWEEP_SHAPE (dev A/B) picks another shape
    const char* se = getenv("ALIPMPC_SWEEP_SHAPE");
    const int shape = se ? atoi(se) : SWEEP_SHAPE_DEFAULT;
    // measured (profiles/r2/sweep/shapes.txt, B = 65,536): 64 x 1 0.0837 ms (one wave per SIMD: the LDS of a
    // 64-instance chunk), 32 x 2 0.0759 ms (two per SIMD, 2048 waves), 16 x 4 0.106 ms (232 VGPRs cap the SIMD at
    // two waves, and each wave repeats the set-up for a quarter of the instances)
    if (shape == 641)
        launch_sweep_t<NC, FEN, 64, 1>(P, st);
    else
        launch_sweep_t<NC, FEN, 32, 2>(P, st);
}
hipError_t launch_sweep(int nc, bool fen, const KP& P, hipStream_t st)
{
#define SWCASE(K)                                              \
    case K:                                                    \
        fen ? launch_sweep_s<K, true>(P, st) : launch_sweep_s<K, false>(P, st); \
        break;
    switch (nc) {
        SWCASE(0) SWCASE(1) SWCASE(2) SWCASE(3) SWCASE(4) SWCASE(5) SWCASE(6)
    default:
        return hipErrorInvalidValue;
    }
#undef SWCASE
    return hipGetLastError();
}
#endif
