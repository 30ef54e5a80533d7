// U-Net self-attention (reference proc_unet_modern.py:292-317) without the N x N score matrix.
//
// The reference's softmax runs over the QUERY index i for each key j (attn.softmax(dim=1) on [b, i, j, h]):
//   P[i][j] = exp(scale q_i.k_j - lse_j),  lse_j = log sum_i exp(scale q_i.k_j),  out_i = sum_j P[i][j] v_j.
// A column's statistics need every query, so they are a pass of their own (nps_attn_colstats: per key tile, a
// stream over query tiles with an online column max / sum); the forward then knows the final lse_j and needs no
// running rescale.  Backward (softmax over i):
//   dV_j = sum_i P[i][j] dO_i,  delta_j = dV_j.v_j,  dS[i][j] = P[i][j] (dO_i.v_j - delta_j),
//   dK_j = scale sum_i dS[i][j] q_i,  dQ_i = scale sum_j dS[i][j] k_j,
// as a key-tile kernel (dV, delta, dK; P recomputed from lse) and a query-tile kernel (dQ).
//
// All contractions run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  Tensors are read
// and written in the projection's own layout: qkv / dqkv [B][N][heads][q | k | v] (dk each), out / dout
// [B][N][heads * dk], lse / delta [B][heads][N].
//
// Work-group = 256 threads = 4 waves = one 64-row tile (queries or keys) of one (batch, head), streaming 64-row
// tiles of the other index.  Operands pass through LDS in 64-wide head-dimension chunks ([64][64 + 4] fp32, the
// +4 keeps 16-byte row reads conflict-free); the chunk after the current one is already in flight in registers
// while the MFMAs of the current one run.  Wave w owns rows [16w, 16w + 16) of the work-group's tile:
//   S-type  (A [m][d] . B [n][d]^T):  lane (r = lane & 15, g = lane >> 4) reads 4 consecutive d of its A row
//           and of the B rows 16t + r as one 16-byte LDS read each and feeds them to 4 MFMAs (both operands use
//           the same d -> k assignment, so the sum is the same); D: row 16w + 4g + reg, column 16t + r.
//   PV-type (P [m][k] . B [k][n]):    P goes registers -> LDS (row-major for the query-tile kernels, transposed
//           for the key-tile ones) and comes back as the A operand; B rows are read one float per lane.
// Tails: rows >= N and head-dimension columns >= dk are zero in LDS (so no stale NaN can reach an MFMA) AND the
// scores are masked where it matters: a padded query row gets -inf before a column max / sum and P = 0 before
// any product with dO or Q; a padded key column gets P = 0; nothing outside [0, N) x [0, dk) is stored.
#include "nps_common.hpp"

namespace {

constexpr int AT = 64;       // tile rows
constexpr int ADC = 64;      // head-dimension chunk
constexpr int ALD = ADC + 4;  // LDS row stride (floats)
constexpr int ATTN_MAX_DK = 256;

typedef float (*tile_t)[ALD];

// 64 x 64 chunk <- rows [row0, row0 + 64) x columns [d0, d0 + 64) of a [N][rstride] matrix: 4 16-byte pieces
// per thread, zero outside [0, N) x [0, dk)
__device__ __forceinline__ void fetch(f32x4 (&r)[4], const float* __restrict__ base, long rstride, int row0, int N,
                                      int d0, int dk, int tid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k;
        const int n = row0 + (p >> 4), d = d0 + (p & 15) * 4;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        r[k] = (n < N && d < dk) ? *reinterpret_cast<const f32x4*>(base + (long)n * rstride + d) : z;
    }
}

__device__ __forceinline__ void stash(tile_t s, const f32x4 (&r)[4], int tid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k;
        *reinterpret_cast<f32x4*>(&s[p >> 4][(p & 15) * 4]) = r[k];
    }
}

// acc[t] += A[16w + .][:] . B[16t + .][:]^T over the chunk's 64 columns
__device__ __forceinline__ void gemm_nt(f32x4 (&acc)[4], const tile_t As, const tile_t Bs, int wave, int r, int g) {
#pragma unroll
    for (int kk = 0; kk < ADC / 16; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&As[16 * wave + r][kk * 16 + 4 * g]);
        f32x4 bq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bq[t] = *reinterpret_cast<const f32x4*>(&Bs[16 * t + r][kk * 16 + 4 * g]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bq[t][s], acc[t], 0, 0, 0);
    }
}

// o[t] += P[16w + .][k] . B[k][16t + .] over k < 64
__device__ __forceinline__ void gemm_pv(f32x4 (&o)[4], const tile_t Ps, const tile_t Bs, int wave, int r, int g) {
#pragma unroll
    for (int kk = 0; kk < AT / 16; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&Ps[16 * wave + r][kk * 16 + 4 * g]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], Bs[kk * 16 + 4 * g + s][16 * t + r], o[t], 0, 0, 0);
    }
}

template <int NDC>
__device__ __forceinline__ void gemm_pv_chunk(f32x4 (&o)[NDC][4], int c, const tile_t Ps, const tile_t Bs, int wave,
                                              int r, int g) {
#pragma unroll
    for (int cc = 0; cc < NDC; ++cc)
        if (cc == c) gemm_pv(o[cc], Ps, Bs, wave, r, g);
}

__device__ __forceinline__ void zero4(f32x4 (&a)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// D-layout accumulators (row 16w + 4g + reg, chunk column 16t + r) -> dst rows [row0, ..) x columns [0, dk)
template <int NDC>
__device__ __forceinline__ void store_acc(const f32x4 (&o)[NDC][4], float* __restrict__ dst, long rstride, int row0,
                                          int N, int dk, float mul, int wave, int r, int g) {
#pragma unroll
    for (int c = 0; c < NDC; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int d = c * ADC + 16 * t + r;
            if (d >= dk) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = row0 + 16 * wave + 4 * g + e;
                if (n < N) dst[(long)n * rstride + d] = o[c][t][e] * mul;
            }
        }
}

struct Geo {
    const float *q, *k, *v;  // this (batch, head)'s q / k / v columns of qkv, row stride rs
    long rs;
};

__device__ __forceinline__ Geo geo(const float* qkv, int b, int h, int N, int heads, int dk) {
    Geo G;
    G.rs = (long)heads * 3 * dk;
    G.q = qkv + (long)b * N * G.rs + (long)h * 3 * dk;
    G.k = G.q + dk;
    G.v = G.q + 2 * dk;
    return G;
}

// ---- column statistics: lse[b][h][j] = log sum_i exp(scale q_i.k_j) ----
__global__ __launch_bounds__(256) void attn_colstats_kernel(const float* __restrict__ qkv, float* __restrict__ lse,
                                                            int N, int heads, int dk, float scale) {
    __shared__ __attribute__((aligned(16))) float As[AT][ALD], Bs[AT][ALD];
    __shared__ float red_m[4][AT], red_l[4][AT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.x * AT, h = blockIdx.y, b = blockIdx.z;
    const Geo G = geo(qkv, b, h, N, heads, dk);
    const int nc = (dk + ADC - 1) / ADC, ntile = (N + AT - 1) / AT;
    float m[4], l[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) m[t] = -INFINITY, l[t] = 0.f;
    f32x4 ra[4], rb[4];
    fetch(ra, G.q, G.rs, 0, N, 0, dk, tid);
    fetch(rb, G.k, G.rs, j0, N, 0, dk, tid);
    for (int it = 0; it < ntile; ++it) {
        f32x4 s[4];
        zero4(s);
        for (int ph = 0; ph < nc; ++ph) {
            __syncthreads();
            stash(As, ra, tid);
            stash(Bs, rb, tid);
            __syncthreads();
            int nph = ph + 1, nit = it;
            if (nph == nc) nph = 0, ++nit;
            if (nit < ntile) {
                fetch(ra, G.q, G.rs, nit * AT, N, nph * ADC, dk, tid);
                fetch(rb, G.k, G.rs, j0, N, nph * ADC, dk, tid);
            }
            gemm_nt(s, As, Bs, wave, r, g);
        }
        // online column max / sum over this wave's 16 query rows; padded rows are -inf
        const int ibase = it * AT + 16 * wave + 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v[4], mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = (ibase + e < N) ? s[t][e] * scale : -INFINITY;
                mx = fmaxf(mx, v[e]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // branch-free: a column with no row yet (mn = -inf: this wave's rows are all padding so far) keeps
            // l = 0 — every exponent below is then -inf - 0
            const float mn = fmaxf(m[t], mx), ms = mn > -INFINITY ? mn : 0.f;
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += expf(v[e] - ms);  // exp(-inf) = 0 for padded rows
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            l[t] = l[t] * expf(m[t] - ms) + sum;
            m[t] = mn;
        }
    }
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) red_m[wave][16 * t + r] = m[t], red_l[wave][16 * t + r] = l[t];
    }
    __syncthreads();
    if (tid < AT && j0 + tid < N) {
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = fmaxf(M, red_m[w][tid]);
        float L = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (red_m[w][tid] > -INFINITY) L += red_l[w][tid] * expf(red_m[w][tid] - M);
        lse[((long)b * heads + h) * N + j0 + tid] = M + logf(L);
    }
}

// ---- forward: out_i = sum_j exp(scale q_i.k_j - lse_j) v_j ----
template <int NDC>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                       float* __restrict__ out, int N, int heads, int dk,
                                                       float scale) {
    __shared__ __attribute__((aligned(16))) float As[AT][ALD], Bs[AT][ALD], Ps[AT][ALD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * AT, h = blockIdx.y, b = blockIdx.z;
    const Geo G = geo(qkv, b, h, N, heads, dk);
    const float* lse_bh = lse + ((long)b * heads + h) * N;
    const int nc = (dk + ADC - 1) / ADC, ntile = (N + AT - 1) / AT;
    f32x4 o[NDC][4];
#pragma unroll
    for (int c = 0; c < NDC; ++c) zero4(o[c]);
    f32x4 ra[4], rb[4];
    auto prefetch = [&](int jt, int ph) {
        if (ph < nc) {
            fetch(ra, G.q, G.rs, i0, N, ph * ADC, dk, tid);
            fetch(rb, G.k, G.rs, jt * AT, N, ph * ADC, dk, tid);
        } else {
            fetch(rb, G.v, G.rs, jt * AT, N, (ph - nc) * ADC, dk, tid);
        }
    };
    prefetch(0, 0);
    for (int jt = 0; jt < ntile; ++jt) {
        f32x4 s[4];
        zero4(s);
        for (int ph = 0; ph < 2 * nc; ++ph) {
            __syncthreads();
            if (ph < nc) stash(As, ra, tid);
            stash(Bs, rb, tid);
            __syncthreads();
            int nph = ph + 1, njt = jt;
            if (nph == 2 * nc) nph = 0, ++njt;
            if (njt < ntile) prefetch(njt, nph);
            if (ph < nc) {
                gemm_nt(s, As, Bs, wave, r, g);
                if (ph == nc - 1) {
                    // P for this wave's 16 query rows (read back by this wave only); padded keys are 0
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int j = jt * AT + 16 * t + r;
                        const float lj = j < N ? lse_bh[j] : 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            Ps[16 * wave + 4 * g + e][16 * t + r] = j < N ? expf(s[t][e] * scale - lj) : 0.f;
                    }
                }
            } else {
                gemm_pv_chunk<NDC>(o, ph - nc, Ps, Bs, wave, r, g);
            }
        }
    }
    store_acc<NDC>(o, out + (long)b * N * heads * dk + (long)h * dk, (long)heads * dk, i0, N, dk, 1.f, wave, r, g);
}

// ---- backward, key tile: dV, delta, dK ----
// (both backward kernels are bounded to 256 registers, __launch_bounds__(256, 2): two work-groups per CU hide each
// other's barriers and chunk loads — measured 26.0 -> 17.5 ms at B = 2, N = 16129, dk = 192 against one per CU)
template <int NDC>
__global__ __launch_bounds__(256, 2) void attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                          const float* __restrict__ dout, float* __restrict__ dqkv,
                                                          float* __restrict__ delta, int N, int heads, int dk,
                                                          float scale) {
    __shared__ __attribute__((aligned(16))) float As[AT][ALD], Bs[AT][ALD], Pt[AT][ALD];
    __shared__ float delta_s[AT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int j0 = blockIdx.x * AT, h = blockIdx.y, b = blockIdx.z;
    const Geo G = geo(qkv, b, h, N, heads, dk);
    const long os = (long)heads * dk;
    const float* dO = dout + (long)b * N * os + (long)h * dk;
    float* dq = dqkv + (long)b * N * G.rs + (long)h * 3 * dk;
    const int nc = (dk + ADC - 1) / ADC, ntile = (N + AT - 1) / AT;
    float lj[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) lj[t] = (j0 + 16 * t + r < N) ? lse[((long)b * heads + h) * N + j0 + 16 * t + r] : 0.f;
    f32x4 acc[NDC][4];
#pragma unroll
    for (int c = 0; c < NDC; ++c) zero4(acc[c]);
    f32x4 ra[4], rb[4];

    // P^T (or dS^T) of the current (query tile, key tile): lane holds rows i = 16w + 4g + e of column 16t + r,
    // four consecutive i of one key row -> one 16-byte store.  Padded queries and keys are 0.
    auto put_t = [&](const f32x4 (&p)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(&Pt[16 * t + r][16 * wave + 4 * g]) = p[t];
    };

    // pass 1: dV_j = sum_i P[i][j] dO_i
    auto prefetch1 = [&](int it, int ph) {
        if (ph < nc) {
            fetch(ra, G.q, G.rs, it * AT, N, ph * ADC, dk, tid);
            fetch(rb, G.k, G.rs, j0, N, ph * ADC, dk, tid);
        } else {
            fetch(rb, dO, os, it * AT, N, (ph - nc) * ADC, dk, tid);
        }
    };
    prefetch1(0, 0);
    for (int it = 0; it < ntile; ++it) {
        f32x4 s[4];
        zero4(s);
        for (int ph = 0; ph < 2 * nc; ++ph) {
            __syncthreads();
            if (ph < nc) stash(As, ra, tid);
            stash(Bs, rb, tid);
            __syncthreads();
            int nph = ph + 1, nit = it;
            if (nph == 2 * nc) nph = 0, ++nit;
            if (nit < ntile) prefetch1(nit, nph);
            if (ph < nc) {
                gemm_nt(s, As, Bs, wave, r, g);
                if (ph == nc - 1) {
                    f32x4 p[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool ok = (it * AT + 16 * wave + 4 * g + e < N) && (j0 + 16 * t + r < N);
                            p[t][e] = ok ? expf(s[t][e] * scale - lj[t]) : 0.f;
                        }
                    put_t(p);
                }
            } else {
                gemm_pv_chunk<NDC>(acc, ph - nc, Pt, Bs, wave, r, g);
            }
        }
    }
    store_acc<NDC>(acc, dq + 2 * dk, G.rs, j0, N, dk, 1.f, wave, r, g);
    // delta_j = dV_j . v_j for this wave's key rows 16w + 4g + e
    {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NDC; ++c)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int d = c * ADC + 16 * t + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + 16 * wave + 4 * g + e;
                    if (d < dk && j < N) part[e] += acc[c][t][e] * G.v[(long)j * G.rs + d];
                }
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) part[e] += __shfl_xor(part[e], o, 64);
            const int jl = 16 * wave + 4 * g + e;
            if (r == 0) {
                delta_s[jl] = part[e];
                if (j0 + jl < N) delta[((long)b * heads + h) * N + j0 + jl] = part[e];
            }
        }
    }
    __syncthreads();
    float dj[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dj[t] = delta_s[16 * t + r];
#pragma unroll
    for (int c = 0; c < NDC; ++c) zero4(acc[c]);

    // pass 2: dK_j = scale sum_i P[i][j] (dO_i.v_j - delta_j) q_i
    auto prefetch2 = [&](int it, int ph) {
        if (ph < nc) {
            fetch(ra, G.q, G.rs, it * AT, N, ph * ADC, dk, tid);
            fetch(rb, G.k, G.rs, j0, N, ph * ADC, dk, tid);
        } else if (ph < 2 * nc) {
            fetch(ra, dO, os, it * AT, N, (ph - nc) * ADC, dk, tid);
            fetch(rb, G.v, G.rs, j0, N, (ph - nc) * ADC, dk, tid);
        } else {
            fetch(rb, G.q, G.rs, it * AT, N, (ph - 2 * nc) * ADC, dk, tid);
        }
    };
    prefetch2(0, 0);
    for (int it = 0; it < ntile; ++it) {
        f32x4 s[4], dp[4];
        zero4(s);
        zero4(dp);
        for (int ph = 0; ph < 3 * nc; ++ph) {
            __syncthreads();
            if (ph < 2 * nc) stash(As, ra, tid);
            stash(Bs, rb, tid);
            __syncthreads();
            int nph = ph + 1, nit = it;
            if (nph == 3 * nc) nph = 0, ++nit;
            if (nit < ntile) prefetch2(nit, nph);
            if (ph < nc) {
                gemm_nt(s, As, Bs, wave, r, g);
            } else if (ph < 2 * nc) {
                gemm_nt(dp, As, Bs, wave, r, g);
                if (ph == 2 * nc - 1) {
                    f32x4 ds[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool ok = (it * AT + 16 * wave + 4 * g + e < N) && (j0 + 16 * t + r < N);
                            ds[t][e] = ok ? expf(s[t][e] * scale - lj[t]) * (dp[t][e] - dj[t]) : 0.f;
                        }
                    put_t(ds);
                }
            } else {
                gemm_pv_chunk<NDC>(acc, ph - 2 * nc, Pt, Bs, wave, r, g);
            }
        }
    }
    store_acc<NDC>(acc, dq + dk, G.rs, j0, N, dk, scale, wave, r, g);
}

// ---- backward, query tile: dQ_i = scale sum_j P[i][j] (dO_i.v_j - delta_j) k_j ----
template <int NDC>
__global__ __launch_bounds__(256, 2) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                         const float* __restrict__ dout, float* __restrict__ dqkv,
                                                         const float* __restrict__ delta, int N, int heads, int dk,
                                                         float scale) {
    __shared__ __attribute__((aligned(16))) float As[AT][ALD], Bs[AT][ALD], Ps[AT][ALD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * AT, h = blockIdx.y, b = blockIdx.z;
    const Geo G = geo(qkv, b, h, N, heads, dk);
    const long os = (long)heads * dk;
    const float* dO = dout + (long)b * N * os + (long)h * dk;
    const float* lse_bh = lse + ((long)b * heads + h) * N;
    const float* delta_bh = delta + ((long)b * heads + h) * N;
    const int nc = (dk + ADC - 1) / ADC, ntile = (N + AT - 1) / AT;
    f32x4 acc[NDC][4];
#pragma unroll
    for (int c = 0; c < NDC; ++c) zero4(acc[c]);
    f32x4 ra[4], rb[4];
    auto prefetch = [&](int jt, int ph) {
        if (ph < nc) {
            fetch(ra, G.q, G.rs, i0, N, ph * ADC, dk, tid);
            fetch(rb, G.k, G.rs, jt * AT, N, ph * ADC, dk, tid);
        } else if (ph < 2 * nc) {
            fetch(ra, dO, os, i0, N, (ph - nc) * ADC, dk, tid);
            fetch(rb, G.v, G.rs, jt * AT, N, (ph - nc) * ADC, dk, tid);
        } else {
            fetch(rb, G.k, G.rs, jt * AT, N, (ph - 2 * nc) * ADC, dk, tid);
        }
    };
    prefetch(0, 0);
    for (int jt = 0; jt < ntile; ++jt) {
        f32x4 s[4], dp[4];
        zero4(s);
        zero4(dp);
        for (int ph = 0; ph < 3 * nc; ++ph) {
            __syncthreads();
            if (ph < 2 * nc) stash(As, ra, tid);
            stash(Bs, rb, tid);
            __syncthreads();
            int nph = ph + 1, njt = jt;
            if (nph == 3 * nc) nph = 0, ++njt;
            if (njt < ntile) prefetch(njt, nph);
            if (ph < nc) {
                gemm_nt(s, As, Bs, wave, r, g);
            } else if (ph < 2 * nc) {
                gemm_nt(dp, As, Bs, wave, r, g);
                if (ph == 2 * nc - 1) {
                    // dS for this wave's 16 query rows (read back by this wave only); padded keys are 0
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int j = jt * AT + 16 * t + r;
                        const float lj = j < N ? lse_bh[j] : 0.f, dj = j < N ? delta_bh[j] : 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            Ps[16 * wave + 4 * g + e][16 * t + r] =
                                j < N ? expf(s[t][e] * scale - lj) * (dp[t][e] - dj) : 0.f;
                    }
                }
            } else {
                gemm_pv_chunk<NDC>(acc, ph - 2 * nc, Ps, Bs, wave, r, g);
            }
        }
    }
    store_acc<NDC>(acc, dqkv + (long)b * N * G.rs + (long)h * 3 * dk, G.rs, i0, N, dk, scale, wave, r, g);
}

int check_shape(const char* what, int B, int N, int heads, int dk) {
    NPS_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1, "%s: B, N, heads must be >= 1 (got %d, %d, %d)", what, B, N, heads);
    NPS_CHECK_ARG(dk >= 4 && dk % 4 == 0 && dk <= ATTN_MAX_DK, "%s: dk must be a multiple of 4 in [4, %d] (got %d)",
                  what, ATTN_MAX_DK, dk);
    NPS_CHECK_ARG(heads <= 65535 && B <= 65535, "%s: heads and B must be <= 65535 (got %d, %d)", what, heads, B);
    NPS_CHECK_ARG((long)B * N * heads * 3 * dk < (1L << 40), "%s: tensor too large", what);
    return 0;
}

}  // namespace

extern "C" int nps_attn_colstats(const float* qkv, float* lse, int B, int N, int heads, int dk, float scale,
                                 void* stream) {
    if (int rc = check_shape("nps_attn_colstats", B, N, heads, dk)) return rc;
    NPS_CHECK_ARG(qkv && lse, "nps_attn_colstats: NULL tensor");
    const dim3 grid((N + AT - 1) / AT, heads, B);
    attn_colstats_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(qkv, lse, N, heads, dk, scale);
    NPS_CHECK_LAUNCH("nps_attn_colstats");
    return 0;
}

extern "C" int nps_attn_fwd(const float* qkv, const float* lse, float* out, int B, int N, int heads, int dk,
                            float scale, void* stream) {
    if (int rc = check_shape("nps_attn_fwd", B, N, heads, dk)) return rc;
    NPS_CHECK_ARG(qkv && lse && out, "nps_attn_fwd: NULL tensor");
    const dim3 grid((N + AT - 1) / AT, heads, B);
    hipStream_t s = (hipStream_t)stream;
    switch ((dk + ADC - 1) / ADC) {
        case 1: attn_fwd_kernel<1><<<grid, 256, 0, s>>>(qkv, lse, out, N, heads, dk, scale); break;
        case 2: attn_fwd_kernel<2><<<grid, 256, 0, s>>>(qkv, lse, out, N, heads, dk, scale); break;
        case 3: attn_fwd_kernel<3><<<grid, 256, 0, s>>>(qkv, lse, out, N, heads, dk, scale); break;
        default: attn_fwd_kernel<4><<<grid, 256, 0, s>>>(qkv, lse, out, N, heads, dk, scale); break;
    }
    NPS_CHECK_LAUNCH("nps_attn_fwd");
    return 0;
}

extern "C" size_t nps_attn_bwd_ws_floats(int B, int N, int heads, int dk) {
    (void)dk;
    if (B < 1 || N < 1 || heads < 1) return 0;
    return (size_t)B * heads * N;  // delta[b][h][j]
}

extern "C" int nps_attn_bwd(const float* qkv, const float* lse, const float* dout, float* dqkv, float* ws, int B,
                            int N, int heads, int dk, float scale, void* stream) {
    if (int rc = check_shape("nps_attn_bwd", B, N, heads, dk)) return rc;
    NPS_CHECK_ARG(qkv && lse && dout && dqkv && ws, "nps_attn_bwd: NULL tensor");
    const dim3 grid((N + AT - 1) / AT, heads, B);
    hipStream_t s = (hipStream_t)stream;
#define NPS_ATTN_BWD(NDC)                                                                            \
    attn_bwd_kv_kernel<NDC><<<grid, 256, 0, s>>>(qkv, lse, dout, dqkv, ws, N, heads, dk, scale);     \
    attn_bwd_q_kernel<NDC><<<grid, 256, 0, s>>>(qkv, lse, dout, dqkv, ws, N, heads, dk, scale)
    switch ((dk + ADC - 1) / ADC) {
        case 1: NPS_ATTN_BWD(1); break;
        case 2: NPS_ATTN_BWD(2); break;
        case 3: NPS_ATTN_BWD(3); break;
        default: NPS_ATTN_BWD(4); break;
    }
#undef NPS_ATTN_BWD
    NPS_CHECK_LAUNCH("nps_attn_bwd");
    return 0;
}
