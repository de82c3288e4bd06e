// dataset.inc — imitation-learning rows of the closed loop (alipmpc_closed_loop_dataset_batch, include/alipmpc.h).
// Included by alipmpc.hip in the ALIP_PART == 0 unit.
//
// The loop's kernels stage, per tick that ran, the DS_TICK values only they see (cl_update_kernel: plant state
// before the tick, planned foothold, x_nex, v_des_map before its update) and per step the DS_STEP values (stance
// foot, heading input, leg_ind, touchdown state) into dense B x S x f_cyc / B x S areas of the call's workspace.
// After the episode groups have joined, two kernels on the call's stream turn them into the reference's rows
// (data_procs/logger_iml.py:377-401 X / y_mpc, :416-428 y_act):
//   ds_scan_kernel     row_start = exclusive int64 scan of f_cyc * (steps entered); one workgroup walks the batch
//                      in tiles of DS_SCAN_TILE: 4 counts per thread, a shuffle scan per wavefront, the 16 wave
//                      totals through the LDS, and a running carry between tiles.
//   ds_compact_kernel  one wavefront per episode.  An episode's rows are one contiguous block of each output, and
//                      the lanes walk it element by element (row and column from the element index), each gathering
//                      its element from the staging, the per-step values, cir / elp / goal or constants — so
//                      a store instruction of the wave writes one contiguous run: 64 x 16 B where the block is
//                      16-byte aligned (after peeling one leading element if it is not), 64 x 8 B at the odd end.
//                      The obstacle columns come straight from the inputs.
// Rows at positions >= max_rows are not written; row_start is always complete.
namespace alip {

struct DsP {
    long long B, max_rows;
    int S, f, nc_max, ne_max;
    double safe, T, Td;        // safe_dis; step time; T / f_cyc
    const double* tick;        // B x S x f x DS_TICK
    const double* step;        // B x S x DS_STEP
    const int32_t* stt;        // B x S x f status of every tick
    const double* cir;
    const int32_t* nc;
    const double* elp;
    const int32_t* ne;
    const double* goal;
    const long long* row_start;
    double* X;
    double* y_mpc;
    double* y_act;
    int32_t* row_status;
};

constexpr int DS_SCAN_THREADS = 1024, DS_SCAN_PER = 4, DS_SCAN_TILE = DS_SCAN_THREADS * DS_SCAN_PER;

__global__ __launch_bounds__(DS_SCAN_THREADS) void ds_scan_kernel(const int32_t* nst, long long B, int f,
                                                                  long long* row_start)
{
    __shared__ long long wtot[DS_SCAN_THREADS / WAVE];
    const int t = threadIdx.x, lane = t % WAVE, w = t / WAVE;
    long long carry = 0;
    for (long long base = 0; base < B; base += DS_SCAN_TILE) {
        const long long i0 = base + (long long)t * DS_SCAN_PER;
        long long c[DS_SCAN_PER], mine = 0;
#pragma unroll
        for (int k = 0; k < DS_SCAN_PER; ++k) {
            c[k] = i0 + k < B ? (long long)f * nst[i0 + k] : 0;
            mine += c[k];
        }
        long long inc = mine;   // inclusive scan over the wavefront
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const long long o = __shfl_up(inc, d, WAVE);
            if (lane >= d) inc += o;
        }
        if (lane == WAVE - 1) wtot[w] = inc;
        __syncthreads();
        long long before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < DS_SCAN_THREADS / WAVE; ++k) {
            const long long v = wtot[k];
            before += k < w ? v : 0;
            tile += v;
        }
        long long run = carry + before + inc - mine;
#pragma unroll
        for (int k = 0; k < DS_SCAN_PER; ++k) {
            if (i0 + k < B) row_start[i0 + k] = run;
            run += c[k];
        }
        carry += tile;
        __syncthreads();
    }
    if (t == 0) row_start[B] = carry;
}

// rest_t = T - i (T / f_cyc) (main_sim_mpc.py:78) with each operation rounded on its own, as the host rounds it
__device__ inline double ds_rest_t(double T, double Td, unsigned i)
{
#pragma clang fp contract(off)
    const double d = (double)i * Td;
    return T - d;
}

// the wave stores elements 0 .. n-1 of a contiguous block: get(e) is element e
template <class F>
__device__ inline void ds_walk(double* base, unsigned n, int lane, F get)
{
    if (n == 0) return;
    unsigned e0 = 0;
    if ((uintptr_t)base & 8) {   // 8- but not 16-byte aligned: one leading element on its own
        if (lane == 0) base[0] = get(0u);
        e0 = 1;
    }
    const unsigned pairs = (n - e0) / 2;
    double2* p2 = reinterpret_cast<double2*>(base + e0);
    for (unsigned q = lane; q < pairs; q += WAVE) {
        double2 v;
        v.x = get(e0 + 2 * q);
        v.y = get(e0 + 2 * q + 1);
        p2[q] = v;
    }
    if (((n - e0) & 1u) && lane == 0) base[n - 1] = get(n - 1);
}

__global__ __launch_bounds__(256) void ds_compact_kernel(DsP D)
{
    const long long b = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (b >= D.B) return;
    const int lane = threadIdx.x % WAVE;
    const long long r0 = D.row_start[b];
    long long rows = D.row_start[b + 1] - r0;
    if (r0 + rows > D.max_rows) rows = D.max_rows - r0;   // the capacity rule
    if (rows <= 0) return;
    const unsigned nr = (unsigned)rows, f = (unsigned)D.f;
    const unsigned n3 = 3u * D.nc_max, n5 = 5u * D.ne_max, ncx = n3 + n5 + 11u;
    const double* tk = D.tick + (size_t)b * D.S * D.f * DS_TICK;   // row r of the episode is tick r of its staging
    const double* sp = D.step + (size_t)b * D.S * DS_STEP;
    if (D.X) {
        const double* cir = D.cir + (size_t)b * n3;
        const double* elp = D.elp + (size_t)b * n5;
        const unsigned ncb = n3 ? 3u * (unsigned)min(max(D.nc[b], 0), D.nc_max) : 0u;
        const unsigned neb = n5 ? 5u * (unsigned)min(max(D.ne[b], 0), D.ne_max) : 0u;
        const double gx = D.goal[2 * b], gy = D.goal[2 * b + 1];
        ds_walk(D.X + (size_t)r0 * ncx, nr * ncx, lane, [&](unsigned e) -> double {
            const unsigned r = e / ncx, c = e - r * ncx;
            if (c < n3) return c < ncb ? cir[c] - (c % 3u == 2u ? D.safe : 0.0) : 0.0;
            if (c < n3 + n5) {
                const unsigned k = c - n3, j = k % 5u;
                return k < neb ? elp[k] - (j == 2u || j == 3u ? D.safe : 0.0) : 0.0;
            }
            const unsigned k = c - n3 - n5, s = r / f;
            if (k < 5u) return tk[(size_t)r * DS_TICK + k];
            if (k < 7u) return sp[s * DS_STEP + (k - 5u)];
            if (k < 9u) return k == 7u ? gx : gy;
            if (k == 9u) return sp[s * DS_STEP + 3];
            return ds_rest_t(D.T, D.Td, r - s * f);
        });
    }
    if (D.y_mpc)
        ds_walk(D.y_mpc + (size_t)r0 * 8, nr * 8u, lane, [&](unsigned e) -> double {
            const unsigned r = e / 8u, c = e % 8u;
            if (c == 2u) return 0.0;
            if (c == 3u) return sp[(r / f) * DS_STEP + 2];
            return tk[(size_t)r * DS_TICK + (c < 2u ? 5u + c : 3u + c)];   // foothold 5, 6; x_nex 7, 8; v_des 9, 10
        });
    if (D.y_act)
        ds_walk(D.y_act + (size_t)r0 * 8, nr * 8u, lane, [&](unsigned e) -> double {
            const unsigned r = e / 8u, c = e % 8u, s = r / f;
            if (c == 2u) return 0.0;
            if (c < 2u) return tk[(size_t)(s * f + f - 1u) * DS_TICK + 5u + c];   // the step's last planned foothold
            if (c == 3u) return sp[s * DS_STEP + 8];
            return sp[s * DS_STEP + c];   // touchdown position 4, 5 and velocity 6, 7
        });
    if (D.row_status) {
        const int32_t* src = D.stt + (size_t)b * D.S * D.f;
        int32_t* dst = D.row_status + r0;
        for (unsigned r = lane; r < nr; r += WAVE) dst[r] = src[r];
    }
}

}  // namespace alip
