// scipy's linear_sum_assignment on the device, one wave per problem: the one solver of the tracker's Hungarian sweep
// (csrc/trackops.hip, d_track_hungarian) and of the MOT walk (csrc/moteval.hip, k_mot_events), and the wave primitives
// under it.
//
// The algorithm is scipy/optimize/rectangular_lsap/rectangular_lsap.cpp (shortest augmenting paths in fp64; the CALLER
// transposes a matrix with more rows than columns, as scipy does) restated step for step, INCLUDING how it breaks ties,
// because which of several optimal assignments comes out decides the tracks and the id switches: the scan over the
// `remaining` columns keeps the first column of minimal reduced cost unless a later one of equal cost is unassigned (then
// the last such), and `remaining` is filled in reverse and compacted by moving its last entry into the hole.  The scan's
// sequential rule is two wave reductions over positions.
//
// A cost is read through a functor: Cost::at(row, col) returns the fp64 cost of the problem's entry.  The solvers'
// arithmetic is additions and subtractions only; contraction is switched off inside their bodies all the same, so that
// they mean the same in a translation unit compiled with contraction and in one without.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tmpnn {

__device__ __forceinline__ void wave_sync() {          // LDS writes of this wave visible to its other lanes (one wave only)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Wave-wide minima without the LDS crossbar (__shfl_xor is a ds_bpermute: ~120 cycles a step, five reductions per scan made a
// scan ~3600 cycles): four DPP exchange steps inside each row of 16 lanes (quad_perm xor 1, xor 2, row_half_mirror,
// row_mirror), then the four rows through v_readlane and the scalar unit.  Keys are unsigned: a double goes through the usual
// order-preserving map of its bits.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_step(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t min_step64(uint64_t x) {
    const uint64_t y = ((uint64_t)dpp_step<CTRL>((uint32_t)(x >> 32)) << 32) | dpp_step<CTRL>((uint32_t)x);
    return y < x ? y : x;
}
template <int CTRL>
__device__ __forceinline__ uint32_t min_step32(uint32_t x) { const uint32_t y = dpp_step<CTRL>(x); return y < x ? y : x; }
// minima over a ROW of 16 lanes (the four DPP steps alone: every lane of the row ends up with its row's minimum)
__device__ __forceinline__ uint32_t row_min32(uint32_t x) {
    x = min_step32<0xB1>(x);          // quad_perm [1,0,3,2]
    x = min_step32<0x4E>(x);          // quad_perm [2,3,0,1]
    x = min_step32<0x141>(x);         // row_half_mirror
    return min_step32<0x140>(x);      // row_mirror
}
__device__ __forceinline__ uint64_t row_min64(uint64_t x) {
    x = min_step64<0xB1>(x);
    x = min_step64<0x4E>(x);
    x = min_step64<0x141>(x);
    return min_step64<0x140>(x);
}
// ROWS: rows of 16 lanes that can hold a live key (problems of <= 16 columns: the first row alone -- three pairs of v_readlane less)
template <int ROWS = 4>
__device__ __forceinline__ uint64_t wave_min64(uint64_t x) {
    x = row_min64(x);
    uint64_t m = ~0ull;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint64_t y = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(x >> 32), 16 * r) << 32) | (uint32_t)__builtin_amdgcn_readlane((uint32_t)x, 16 * r);
        m = y < m ? y : m;
    }
    return m;
}
template <int ROWS = 4>
__device__ __forceinline__ uint32_t wave_min32(uint32_t x) {
    x = row_min32(x);
    uint32_t m = ~0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) { const uint32_t y = (uint32_t)__builtin_amdgcn_readlane(x, 16 * r); m = y < m ? y : m; }
    return m;
}
__device__ __forceinline__ uint64_t key_f64(double x) {        // order-preserving: a < b  <=>  key(a) < key(b)   (no NaNs here)
    const uint64_t b = (uint64_t)__double_as_longlong(x + 0.0);           // (-0.0 -> +0.0: scipy compares with ==)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
    const long long b = __double_as_longlong(x);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)b, l));
}

// the row state of a problem of up to MAX rows / columns (a multiple of 64), in LDS
template <int MAX>
struct LsapShared {
    double u[MAX], spc[MAX];
    int col4row[MAX], path[MAX];
    unsigned char SR[MAX];
};

// rows i < nr <= nc <= MAX columns; result in S.col4row[0..nr); false when no augmenting path was found (cannot happen with
// nr <= nc and finite costs: every loop is bounded all the same, a wave never spins).  Lane l owns columns l, l + 64, ...
// (reduced costs, duals, path, position in `remaining` in registers); the row state lives in LDS.
template <int MAX, class Cost>
__device__ bool wave_lsap_solve(LsapShared<MAX>& S, const Cost& C, int nr, int nc, int lane) {
#pragma clang fp contract(off)
    constexpr int K = MAX / 64;                           // columns per lane
    double v[K];
    int r4c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { v[k] = 0.0; r4c[k] = -1; }
    for (int i = lane; i < nr; i += 64) { S.u[i] = 0.0; S.col4row[i] = -1; }
    wave_sync();
    const int KU = (nc + 63) >> 6;                        // column groups in use
    for (int cur = 0; cur < nr; ++cur) {
        double spc[K];
        int path[K], pos[K];
        bool alive[K], scj[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = lane + 64 * k;
            spc[k] = __builtin_huge_val(); path[k] = -1; pos[k] = nc - 1 - j; alive[k] = j < nc; scj[k] = false;
        }
        for (int i = lane; i < nr; i += 64) S.SR[i] = 0;
        wave_sync();
        int i = cur, sink = -1, num_rem = nc;
        double min_val = 0.0;
        while (sink < 0 && num_rem > 0) {
            if (lane == 0) S.SR[i] = 1;
            const double ui = S.u[i];
            double m = __builtin_huge_val();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k < KU && alive[k]) {
                    const double r = min_val + C.at(i, lane + 64 * k) - ui - v[k];
                    if (r < spc[k]) { path[k] = i; spc[k] = r; }
                    m = spc[k] < m ? spc[k] : m;
                }
            }
            // the minimum, then the scan's choice among the columns that attain it: an unassigned one if there is any (the one at
            // the HIGHEST position of `remaining`), else the one at the lowest position -- one key: unassigned first
            const uint64_t mk = wave_min64(key_f64(m));
            uint32_t sel = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < KU && alive[k] && key_f64(spc[k]) == mk) {
                    const uint32_t q = r4c[k] == -1 ? (uint32_t)(MAX - 1 - pos[k]) : (uint32_t)(MAX + pos[k]);
                    sel = q < sel ? q : sel;
                }
            sel = wave_min32(sel);
            const int ipos = sel < (uint32_t)MAX ? MAX - 1 - (int)sel : (int)sel - MAX;
            int jsel = -1, r4sel = -2;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool mine = k < KU && alive[k] && pos[k] == ipos;
                const unsigned long long bal = __ballot(mine);
                if (bal) {                                       // (exactly one column sits at a position)
                    const int src = __ffsll((long long)bal) - 1;
                    jsel = src + 64 * k;
                    r4sel = __builtin_amdgcn_readlane(r4c[k], src);
                    m = readlane_f64(spc[k], src);
                }
            }
            // No live column attains the minimum (sel is all ones, no position matches, jsel stays -1; cannot happen with finite
            // costs): the row is kept, no column leaves, and the count below ends the scan with sink < 0 -- the solver returns
            // false at once.  Selects, not branches: a branch on sel or jsel in this latency-bound loop cost the tracker's
            // 60 x 66 problem 22 % (profiles/wave_lsap_refactor.md).
            min_val = m;
            if (r4sel == -1) sink = jsel; else if (r4sel >= 0) i = r4sel;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (lane + 64 * k == jsel) { scj[k] = true; alive[k] = false; }
                else if (alive[k] && pos[k] == num_rem - 1) pos[k] = ipos;
            }
            num_rem = jsel < 0 ? 0 : num_rem - 1;
        }
        if (sink < 0) return false;
        // dual variables (with col4row as it was BEFORE the augmentation), then the augmentation along `path`
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (lane + 64 * k < nc) { S.spc[lane + 64 * k] = spc[k]; S.path[lane + 64 * k] = path[k]; }
        wave_sync();
        for (int i2 = lane; i2 < nr; i2 += 64)
            if (S.SR[i2]) S.u[i2] += (i2 == cur) ? min_val : (min_val - S.spc[S.col4row[i2]]);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (scj[k]) v[k] -= min_val - spc[k];
        wave_sync();
        int j = sink;
        for (int step = 0;; ++step) {
            if (step > nr) return false;                          // (a path visits a row once: never spin)
            const int ip = S.path[j];
            if (ip < 0 || ip >= nr) return false;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (lane + 64 * k == j) r4c[k] = ip;
            const int old = S.col4row[ip];
            wave_sync();
            if (lane == 0) S.col4row[ip] = j;
            wave_sync();
            j = old;
            if (ip == cur) break;
            if (j < 0 || j >= nc) return false;
        }
    }
    return true;
}

// The same solver for problems of <= 64 columns: lane l is column l AND row l, all state in registers, the only memory traffic
// is the cost row of a scan; rows and columns are addressed with v_readlane / ballots instead of LDS arrays.  ROWS: as in
// wave_min64 (rows of 16 lanes that can hold a column).
template <int ROWS, int MAX, class Cost>
__device__ bool wave_lsap_solve64(LsapShared<MAX>& S, const Cost& C, int nr, int nc, int lane) {
#pragma clang fp contract(off)
    double v = 0.0, u = 0.0;
    int r4c = -1, c4r = -1;
    for (int cur = 0; cur < nr; ++cur) {
        double spc = __builtin_huge_val();
        int path = -1, pos = nc - 1 - lane;
        bool alive = lane < nc, scj = false;
        unsigned long long sr_mask = 0;
        int i = cur, sink = -1, num_rem = nc;
        double min_val = 0.0;
        while (sink < 0 && num_rem > 0) {
            i = __builtin_amdgcn_readfirstlane(i);
            sr_mask |= 1ull << i;
            const double ui = readlane_f64(u, i);
            if (alive) {
                const double r = min_val + C.at(i, lane) - ui - v;
                if (r < spc) { path = i; spc = r; }
            }
            const uint64_t mk = wave_min64<ROWS>(alive ? key_f64(spc) : ~0ull);
            uint32_t sel = 0xFFFFFFFFu;
            if (alive && key_f64(spc) == mk) sel = r4c == -1 ? (uint32_t)(MAX - 1 - pos) : (uint32_t)(MAX + pos);
            sel = wave_min32<ROWS>(sel);
            const int ipos = sel < (uint32_t)MAX ? MAX - 1 - (int)sel : (int)sel - MAX;
            const unsigned long long bal = __ballot(alive && pos == ipos);
            const int jsel = __ffsll((long long)bal) - 1;           // (exactly one column sits at a position)
            const int r4sel = __builtin_amdgcn_readlane(r4c, jsel);
            min_val = readlane_f64(spc, jsel);
            if (r4sel == -1) sink = jsel; else i = r4sel;
            if (lane == jsel) { scj = true; alive = false; }
            else if (alive && pos == num_rem - 1) pos = ipos;
            --num_rem;
        }
        if (sink < 0) return false;                                 // (cannot happen with nr <= nc and finite costs: never spin)
        // dual variables (with the assignment as it was BEFORE the augmentation): row l needs the reduced cost of ITS column
        const double spc_mine = __shfl(spc, c4r < 0 ? 0 : c4r);
        if ((sr_mask >> lane) & 1ull) u += (lane == cur) ? min_val : (min_val - spc_mine);
        if (scj) v -= min_val - spc;
        int j = sink;
        for (;;) {
            const int ip = __builtin_amdgcn_readlane(path, j);
            if (lane == j) r4c = ip;
            const int old = __builtin_amdgcn_readlane(c4r, ip);
            if (lane == ip) c4r = j;
            j = old;
            if (ip == cur) break;
        }
    }
    if (lane < nr) S.col4row[lane] = c4r;
    return true;
}

}  // namespace tmpnn
