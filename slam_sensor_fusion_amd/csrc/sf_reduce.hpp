// sf_reduce.hpp -- the fixed-order float64 reductions of the numerical core: the transposing wave butterfly (swap_add_32 / _16,
// dpp_f64, dpp_keep_add, wave_reduce_32 / _16 / _1), block_reduce_store (a workgroup of BLK threads -> one row of a slab) and
// reduce_partials (a slab -> one record), with the three constants that give them their shape.  No atomics anywhere: the order of
// every sum depends on the launch shape alone, so the result is the same bits run to run.  Like sf_jacobi.hpp it is included INSIDE
// the anonymous namespace of the translation unit that uses it, so the routines keep internal linkage: sf_icp.hip (k_nn_red and its
// kin, k_reduce_solve, sf_cov.hpp, the hooks of sf_icp_testhooks.hpp, which pin every routine: tests/test_gpu_linalg_direct.py) and
// sf_ndt.hip (k_ndt_voxels, k_ndt_derivs, the step and score kernels).  It needs nothing of either and no system header.  The
// one-lane solves are sf_linalg.hpp.
#pragma once

constexpr int BLK = 256;       // threads of a workgroup that calls block_reduce_store
constexpr int REC_STRIDE = 32; // doubles per scan in the exchange buffer

// ------------------------------------------------------------------ reductions
// Wave-level sum of 32 doubles per lane in ~125 VALU instructions and no LDS traffic
// (a plain xor-shuffle reduction of 30 doubles costs 360 ds_bpermute + 180 adds per wave and
// dominated the kernel's instruction issue — profiles/).  Transposing butterfly: at every
// step each lane keeps HALF of its values and adds its partner's copy of that half, so the
// number of live values halves while the number of lanes summed doubles:
//   32 -> 16  partner l ^ 32   v_permlane32_swap   (gfx950)
//   16 ->  8  partner l ^ 16   v_permlane16_swap   (gfx950)
//    8 ->  4  partner l ^ 8    DPP row_ror:8
//    4 ->  2  partner 7-(l&7)  DPP row_half_mirror
//    2 ->  1  partner l ^ 2    DPP quad_perm [2,3,0,1]
//    final    partner l ^ 1    DPP quad_perm [1,0,3,2]
// Afterwards lane l holds the 64-lane total of component (l >> 1).  Fixed order => bitwise
// reproducible.
__device__ __forceinline__ double swap_add_32(double a, double b)
{
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

__device__ __forceinline__ double swap_add_16(double a, double b)
{
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

template <int DPP_CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2loint(v), DPP_CTRL, 0xf, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2hiint(v), DPP_CTRL, 0xf, 0xf, false);
    return __hiloint2double((int)hi, (int)lo);
}

template <int DPP_CTRL>
__device__ __forceinline__ double dpp_keep_add(double a, double b, bool upper)
{
    const double keep = upper ? b : a, give = upper ? a : b;
    return keep + dpp_f64<DPP_CTRL>(give);
}

__device__ __forceinline__ double wave_reduce_32(double (&v)[32])
{
    const int lane = threadIdx.x & 63;
    double w16[16], w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) w16[i] = swap_add_32(v[i], v[i + 16]);
#pragma unroll
    for (int i = 0; i < 8; ++i) w8[i] = swap_add_16(w16[i], w16[i + 8]);
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = dpp_keep_add<0x128>(w8[i], w8[i + 4], (lane & 8) != 0);   // row_ror:8
#pragma unroll
    for (int i = 0; i < 2; ++i) w2[i] = dpp_keep_add<0x141>(w4[i], w4[i + 2], (lane & 4) != 0);   // row_half_mirror
    const double w1 = dpp_keep_add<0x4e>(w2[0], w2[1], (lane & 2) != 0);                          // quad_perm [2,3,0,1]
    return w1 + dpp_f64<0xb1>(w1);                                                                // quad_perm [1,0,3,2]
}

// 16-value form of the same butterfly (half the live registers): afterwards lane l holds the
// 64-lane total of component (l >> 2) & 15.
__device__ __forceinline__ double wave_reduce_16(double (&v)[16])
{
    const int lane = threadIdx.x & 63;
    double w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) w8[i] = swap_add_32(v[i], v[i + 8]);
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = swap_add_16(w8[i], w8[i + 4]);
#pragma unroll
    for (int i = 0; i < 2; ++i) w2[i] = dpp_keep_add<0x128>(w4[i], w4[i + 2], (lane & 8) != 0);   // row_ror:8
    double z = dpp_keep_add<0x141>(w2[0], w2[1], (lane & 4) != 0);                                // row_half_mirror
    z = z + dpp_f64<0x4e>(z);                                                                     // quad_perm [2,3,0,1]
    return z + dpp_f64<0xb1>(z);                                                                  // quad_perm [1,0,3,2]
}

// every lane gets the 64-lane total of one value
__device__ __forceinline__ double wave_reduce_1(double v)
{
    v = swap_add_32(v, v);
    v = swap_add_16(v, v);
    v = v + dpp_f64<0x128>(v);
    v = v + dpp_f64<0x141>(v);
    v = v + dpp_f64<0x4e>(v);
    return v + dpp_f64<0xb1>(v);
}

// Slab layout: partials[(scan * nblocks + block) * 32 + component] — a workgroup's record
// is one contiguous 256-byte row, so both the store here and the column sums below are
// coalesced.
template <int NREC>
__device__ __forceinline__ void block_reduce_store(double (&acc)[NREC], double *__restrict__ dst)
{
    double v[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) v[c] = c < NREC ? acc[c] : 0.0;
    const double total = wave_reduce_32(v);
    __shared__ double s[BLK / 64][32];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((lane & 1) == 0) s[w][lane >> 1] = total;
    __syncthreads();
    if (threadIdx.x < NREC) {
        const int c = threadIdx.x;
        dst[c] = ((s[0][c] + s[1][c]) + s[2][c]) + s[3][c];
    }
}

// Fixed-order sum of one scan's slab by RBLK = 1024 threads: thread (slice s, component c)
// adds rows s, s+32, s+64, ... then the 32 slices are added in order.  Result in rec[]
// (shared).  Deterministic: no atomics, the order depends only on nblocks.
constexpr int RBLK = 1024;
// NT = threads of the calling workgroup (a multiple of 32, at most 1024): with fewer than 1024 a thread takes several
// slices one after the other -- every (slice, component) sum is the same expression, so the result is bit-identical
// for every NT.
template <int NREC, int NT = RBLK>
__device__ __forceinline__ void reduce_partials(const double *__restrict__ part, int nblocks, double *rec)
{
    __shared__ double sl[32][REC_STRIDE + 1];
    const int c = threadIdx.x & 31;
    for (int sidx = threadIdx.x >> 5; sidx < 32; sidx += NT / 32) {
        double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (c < NREC) {
            int b = sidx;
            for (; b + 96 < nblocks; b += 128) {
                const double a0 = part[(size_t)b * REC_STRIDE + c], a1 = part[(size_t)(b + 32) * REC_STRIDE + c];
                const double a2 = part[(size_t)(b + 64) * REC_STRIDE + c], a3 = part[(size_t)(b + 96) * REC_STRIDE + c];
                v0 += a0; v1 += a1; v2 += a2; v3 += a3;
            }
            for (; b < nblocks; b += 32) v0 += part[(size_t)b * REC_STRIDE + c];
        }
        sl[sidx][c] = (v0 + v1) + (v2 + v3);
    }
    __syncthreads();
    if (threadIdx.x < REC_STRIDE) {
        double v = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) v += sl[k][threadIdx.x];
        rec[threadIdx.x] = threadIdx.x < NREC ? v : 0.0;
    }
    __syncthreads();
}
