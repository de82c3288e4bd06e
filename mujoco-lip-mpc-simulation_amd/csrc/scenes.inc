// scenes.inc — counter-based Monte-Carlo scene generator (alipmpc_scenes_batch, include/alipmpc.h).
// Included by alipmpc.hip in the ALIP_PART == 0 unit.
//
// Every output row is a pure function of (seed, global index g, fields, n_cir, n_elp, max_candidates): all
// randomness is U(seed, id, stream, ctr) = splitmix64 of a counter (the finaliser of cl_uniform), so a rank
// generates exactly its shard and nothing is scattered (SURVEY §8e).  The distribution is the reference's random
// obstacle fields (rand_obs.py:31-72, as alipmpc/scenes.py restates them); the stream itself has no reference
// counterpart.  alipmpc/scenes.py: make_batch_counter is the host restatement, bit for bit on everything that
// only uses + - * /, rint and comparisons.
//
// Mapping: one wavefront per instance, no intermediate buffer.  The 64 lanes evaluate candidates c .. c+63 of the
// sequential rejection loop at once and a ballot picks the first acceptable one — the one the sequential rule
// takes.  The later lanes of the round then test the new obstacle only (a candidate rejected by the obstacles
// placed so far stays rejected at the same spacing), so a 5-circle field is usually one round.  The 2000-rejection
// relaxation is applied at its exact position: when tries + (rejections before the next acceptable candidate)
// exceeds 2000, exactly 2001 - tries candidates are consumed, the spacing is halved and the round is evaluated
// again from there.  The placed obstacles live in the wave's LDS row (wave-uniform reads); the initial-state
// pairs are searched the same way, 64 per round.  A field shared by several instances (fields > 0) is recomputed
// by each of them: even a 10-obstacle field is 40-90 rounds, and it needs no allocation, no second launch and no
// dependency between waves.
//
// All decision arithmetic is fp64 with every operation rounded on its own (no FMA contraction): coordinates are
// multiples of 0.01, so near-ties in the rejection tests do occur and a fused multiply-add would flip them.
namespace alip {

constexpr int SC_SEEDS = 2;                              // (10, 10, 0.3) and (0, 0, 1.0): placed first, dropped afterwards
constexpr int SC_MAXO = ALIPMPC_MAX_OBS + SC_SEEDS;      // placed obstacles per field
constexpr int SC_MAXE = ALIPMPC_MAX_OBS / 2;             // ellipses of a mix field
constexpr int SC_MAX_CAND = 1 << 18;                     // hard limit (and default) of max_candidates
constexpr int SC_RELAX = 2000;                           // consecutive rejections before the spacing is halved
constexpr int SC_PAIRS = 1024;                           // initial-state pairs tried (a multiple of 64)
constexpr int SC_CTR_LEG = 4096;                         // stream 2: leg, heading noise (2), vbx, vby follow the pairs

struct ScP {
    long long B, first, fields;
    unsigned long long seed;
    int n_cir, n_elp, nc_max, ne_max, N, max_cand;
    double* x0;
    double* goal;
    int8_t* leg;
    double* cir;
    int32_t* nc;
    double* elp;
    int32_t* ne;
    double* u0;
};

// U(seed, id, stream, ctr) in [0, 1): id < 2^40, stream < 4, ctr < 2^20
__device__ __forceinline__ double sc_uniform(unsigned long long seed, unsigned long long id, int stream, int ctr)
{
    const unsigned long long key = (((id * 4ull + (unsigned long long)stream) << 20) | (unsigned long long)ctr) + 1ull;
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * key;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// np.round(v, 2)
__device__ __forceinline__ double sc_r2(double v)
{
#pragma clang fp contract(off)
    return rint(v * 100.0) / 100.0;
}

__global__ __launch_bounds__(256) void scenes_kernel(ScP P)
{
#pragma clang fp contract(off)
    __shared__ double s_ob[WAVES_PER_BLOCK][SC_MAXO * 3];   // placed [x, y, r], seeds first
    __shared__ double s_el[WAVES_PER_BLOCK][SC_MAXE * 2];   // ellipse j: [b, phi]
    const int lane = lane_id();
    const int w = rfl((int)(threadIdx.x >> 6));
    double* ob = s_ob[w];
    double* el = s_el[w];
    const int tot = P.n_cir + P.n_elp;
    const bool mix = P.n_elp > 0;
    for (long long b = (long long)blockIdx.x * WAVES_PER_BLOCK + w; b < P.B; b += (long long)gridDim.x * WAVES_PER_BLOCK) {
        const unsigned long long g = (unsigned long long)(P.first + b);
        const unsigned long long fid = P.fields > 0 ? g % (unsigned long long)P.fields : g;
        if (lane == 0) {
            ob[0] = 10.0; ob[1] = 10.0; ob[2] = 0.3;
            ob[3] = 0.0; ob[4] = 0.0; ob[5] = 1.0;
        }
        wave_sync();
        // ---- field placement (stream 0): the sequential rejection loop, 64 candidates per round
        int cnt = SC_SEEDS, tries = 0, c = 0;
        double sp2 = 1.6;   // 2 * spacing (halving is exact, so 2 * (spacing / 2) == (2 * spacing) / 2)
        for (int round = 0; round < SC_MAX_CAND && cnt < tot + SC_SEEDS && c < P.max_cand; ++round) {
            const int ci = c + lane;
            const double x = sc_r2(8.5 * sc_uniform(P.seed, fid, 0, 3 * ci));
            const double y = sc_r2(8.5 * sc_uniform(P.seed, fid, 0, 3 * ci + 1));
            const double r = sc_r2(0.65 * sc_uniform(P.seed, fid, 0, 3 * ci + 2) + 0.35);
            auto clears = [&](int k) {   // candidate against placed obstacle k at the current spacing
#pragma clang fp contract(off)
                const double dx = x - ob[3 * k], dy = y - ob[3 * k + 1];
                const double t = (r + ob[3 * k + 2]) + sp2;
                return dx * dx + dy * dy - t * t >= 0.0;
            };
            bool ok = ci < P.max_cand;
            for (int k = 0; k < cnt; ++k) ok = ok && clears(k);
            const int nlive = min(WAVE, P.max_cand - c);
            // Walk the round: candidates c .. c+pos-1 are consumed.  A candidate rejected by the obstacles placed so
            // far stays rejected when more are placed at the same spacing, so after an acceptance the later lanes
            // only test the new obstacle.  A relaxation changes the spacing: the round ends at its exact position.
            int pos = 0;
            for (int it = 0; it < WAVE; ++it) {
                const unsigned long long m = __ballot(ok && lane >= pos);
                const int nrej = (m ? __ffsll((long long)m) - 1 : nlive) - pos;   // rejections before the next acceptable one
                if (tries + nrej > SC_RELAX) {
                    pos += SC_RELAX + 1 - tries;
                    sp2 *= 0.5;
                    tries = 0;
                    break;
                }
                if (!m) {
                    pos = nlive;
                    tries += nrej;
                    break;
                }
                pos += nrej;
                if (lane == pos) {
                    ob[3 * cnt] = x; ob[3 * cnt + 1] = y; ob[3 * cnt + 2] = r;
                }
                wave_sync();
                ++cnt;
                ++pos;
                tries = 0;
                if (cnt == tot + SC_SEEDS || pos >= nlive) break;
                ok = ok && clears(cnt - 1);
            }
            c += pos;
        }
        const int placed = cnt - SC_SEEDS;                       // < tot only when max_candidates ran out
        const int ncn = mix ? (placed + 1) / 2 : placed;         // obstacle i -> circle i/2 (i even) / ellipse (i-1)/2
        const int nen = mix ? placed / 2 : 0;
        // ---- ellipse shapes (stream 1)
        if (lane < nen) {
            const double a = ob[3 * (SC_SEEDS + 2 * lane + 1) + 2];
            const double ha = a / 2;
            el[2 * lane] = sc_r2(ha * sc_uniform(P.seed, fid, 1, 2 * lane) + ha);
            el[2 * lane + 1] = sc_r2(floor(181.0 * sc_uniform(P.seed, fid, 1, 2 * lane + 1)) * (3.141592653589793 / 180.0));
        }
        wave_sync();
        // ---- initial state (stream 2, id = g): first pair outside every inflated obstacle by 0.2
        double px = 0.0, py = 0.0;
        bool found = false;
        for (int rd = 0; rd < SC_PAIRS / WAVE && !found; ++rd) {
            const int i = rd * WAVE + lane;
            px = 10.0 * sc_uniform(P.seed, g, 2, 2 * i);
            py = 10.0 * sc_uniform(P.seed, g, 2, 2 * i + 1);
            bool ok = (px - 10.0) * (px - 10.0) + (py - 10.0) * (py - 10.0) > 0.25;
            for (int k = 0; k < placed; ++k) {
                const double* o = ob + 3 * (SC_SEEDS + k);
                double R = o[2] + 0.4;
                if (mix && (k & 1)) R = fmax(R, el[2 * (k >> 1)] + 0.4);
                R = R + 0.2;
                const double dx = px - o[0], dy = py - o[1];
                ok = ok && (dx * dx + dy * dy >= R * R);
            }
            const unsigned long long m = __ballot(ok);
            found = m != 0;
            const int src = found ? __ffsll((long long)m) - 1 : WAVE - 1;   // none in 1024 pairs: the last pair
            px = __shfl(px, src);
            py = __shfl(py, src);
        }
        // the five remaining draws, one per lane
        const double uf = sc_uniform(P.seed, g, 2, SC_CTR_LEG + (lane < 5 ? lane : 0));
        const double legv = __shfl(uf, 0) < 0.5 ? -1.0 : 1.0;
        const double noise = 0.2 * sqrt(-2.0 * log(1.0 - __shfl(uf, 1))) * cos(2.0 * 3.141592653589793 * __shfl(uf, 2));
        const double vbx = 0.45 + 0.3 * __shfl(uf, 3);
        const double vby = -legv * (0.17 + 0.16 * __shfl(uf, 4));
        const double th = atan2(10.0 - py, 10.0 - px) + noise;
        double sth, cth;
        sincos(th, &sth, &cth);
        const double vx = cth * vbx - sth * vby, vy = sth * vbx + cth * vby;
        // ---- rows (lane j writes element j)
        auto state = [&](int k) { return k == 0 ? px : k == 1 ? py : k == 2 ? vx : k == 3 ? vy : th; };
        if (P.x0 && lane < 5) P.x0[5 * b + lane] = state(lane);
        if (P.goal && lane < 2) P.goal[2 * b + lane] = 10.0;
        if (lane == 0) {
            if (P.leg) P.leg[b] = (int8_t)legv;
            if (P.nc) P.nc[b] = ncn;
            if (P.ne) P.ne[b] = nen;
        }
        if (P.u0)
            for (int j = lane; j < 5 * P.N; j += WAVE) P.u0[(long long)(5 * P.N) * b + j] = state(j % 5);
        if (P.cir)
            for (int j = lane; j < 3 * P.nc_max; j += WAVE) {
                const int slot = j / 3, comp = j - 3 * slot;
                double v = 0.0;
                if (slot < ncn) {
                    v = ob[3 * (SC_SEEDS + (mix ? 2 * slot : slot)) + comp];
                    if (comp == 2) v = v + 0.4;
                }
                P.cir[(long long)(3 * P.nc_max) * b + j] = v;
            }
        if (P.elp)
            for (int j = lane; j < 5 * P.ne_max; j += WAVE) {
                const int slot = j / 5, comp = j - 5 * slot;
                double v = 0.0;
                if (slot < nen) {
                    if (comp < 3) v = ob[3 * (SC_SEEDS + 2 * slot + 1) + comp];
                    else v = el[2 * slot + comp - 3];
                    if (comp == 2 || comp == 3) v = v + 0.4;
                }
                P.elp[(long long)(5 * P.ne_max) * b + j] = v;
            }
        wave_sync();   // the row reads above come before the next instance's placements
    }
}

}  // namespace alip
