// 1-D U-Net convs for gfx950 (MI355X): the k-tap Conv1d along L of channels-last [B][L][C] fp32 activations as an
// implicit GEMM on exact fp32 MFMA (v_mfma_f32_32x32x2_f32), forward (nps_conv1d_fwd: also the transposed conv's two
// phases and every input gradient, with derived weights) and weight gradient (nps_conv1d_wgrad, split reduction with
// a fixed schedule and a reduce pass: no atomics).  See include/nps.h for the semantics.
#include "nps_common.hpp"
#include <cstdint>

namespace {

// ------------------------------------------------------------------------------ forward
// GEMM view: rows = output positions of one sample (tiled along L, a tile never crosses a sample), columns = Cout,
// reduction = K taps x Cin.  A work-group (4 waves) owns 64 positions x 64 output channels, a wave 32 x 32 (two
// accumulators of 16 registers, even and odd channel pairs of a chunk, added at the end).  Per chunk of 16 input channels the frame patch ((64 - 1) S + K positions) is staged
// transposed as Xs[ci][position] and the weights as Ws[tap][ci][co]; MFMA operand A = Xs (lane: position, k: ci),
// B = Ws (lane: co, k: ci), so every ds_read_b32 of a 32-lane half reads 32 consecutive words.  For stride 2 the
// patch row is stored de-interleaved (even positions, then odd ones): position 2 l + t of lanes l is again a run of
// consecutive words.
constexpr int C1_TL = 64, C1_TN = 64, C1_KC = 16;

template <int K, int S>
struct C1Geo {
    static constexpr int XP = (C1_TL - 1) * S + K;            // patch positions
    static constexpr int XH = (XP + 1) / 2;                   // (stride 2) start of the odd half
    static constexpr int XROW = S == 1 ? XP : 2 * XH;
    static constexpr int XPITCH = (XROW + 29) / 32 * 32 + 2;  // = 2 (mod 32): the transposing writes spread over banks
    __device__ static __forceinline__ int xidx(int p) { return S == 1 ? p : (p & 1) * XH + (p >> 1); }
};

// channels [c, c + 4) of frame position f of sample b (zero outside the frame, the sources and Cin)
__device__ __forceinline__ f32x4 c1_load_quad(const nps_conv1d_t& p, int b, int f, int c) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (f < 0 || f >= p.Lc || c >= p.Cin) return v;
    int cb = 0;
#pragma unroll
    for (int i = 0; i < NPS_MAX_SRC; ++i) {
        if (i < p.nsrc) {
            const nps_src1_t s = p.src[i];
            const int ce = cb + s.C;
            const int lp = f - s.off;
            if (c < ce && c + 4 > cb && lp >= 0 && lp < s.L) {
                const float* row = s.ptr + ((size_t)b * s.L + lp) * s.C;
                if (c >= cb && c + 4 <= ce && ((s.C | (c - cb)) & 3) == 0 && ((uintptr_t)s.ptr & 15) == 0) {
                    v = *reinterpret_cast<const f32x4*>(row + (c - cb));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e >= cb && c + e < ce) v[e] = row[c + e - cb];
                }
            }
            cb = ce;
        }
    }
    return v;
}

template <int K, int S>
__global__ __launch_bounds__(256) void conv1d_kernel(const nps_conv1d_t p, int ltiles, int cin_p, int cout_p) {
    using G = C1Geo<K, S>;
    __shared__ __attribute__((aligned(16))) float Xs[C1_KC * G::XPITCH];
    __shared__ __attribute__((aligned(16))) float Ws[K * C1_KC * C1_TN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, j = lane & 31;
    const int b = blockIdx.x / ltiles, l0 = (blockIdx.x % ltiles) * C1_TL;
    const int n0 = blockIdx.y * C1_TN;
    const int f0 = l0 * S - p.pad_l;  // frame position of patch position 0
    // a wave whose 32 rows or 32 columns lie wholly outside the output only takes part in the staging
    const bool active = l0 + wm * 32 < p.Lout && n0 + wn * 32 < p.Cout;

    // two accumulators, even and odd channel pairs of a chunk: each fp32 summation chain is half as long (half the
    // rounding error growth of one sequential chain over K taps x Cin), added once at the end
    f32x16 acc, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc1[r] = 0.f;

    const float* xrow = Xs + h * G::XPITCH;
    const float* wrow = Ws + h * C1_TN + wn * 32 + j;
    for (int c0 = 0; c0 < cin_p; c0 += C1_KC) {
        __syncthreads();
        for (int idx = tid; idx < G::XP * 4; idx += 256) {
            const int pp = idx >> 2, cq = idx & 3;
            const f32x4 v = c1_load_quad(p, b, f0 + pp, c0 + cq * 4);
            float* d = Xs + (cq * 4) * G::XPITCH + G::xidx(pp);
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e * G::XPITCH] = v[e];
        }
#pragma unroll
        for (int t = 0; t < K; ++t) {  // Ws[t][ci][co]: 16 x 64 floats = 256 float4 per tap
            const int ci = tid >> 4, c4 = (tid & 15) * 4;
            *reinterpret_cast<f32x4*>(Ws + (t * C1_KC + ci) * C1_TN + c4) = *reinterpret_cast<const f32x4*>(
                p.wpack + ((size_t)t * cin_p + c0 + ci) * cout_p + n0 + c4);
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int xi = G::xidx((wm * 32 + j) * S + t);
#pragma unroll
                for (int kk = 0; kk < C1_KC / 2; kk += 2) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xrow[kk * 2 * G::XPITCH + xi],
                                                               wrow[(t * C1_KC + kk * 2) * C1_TN], acc, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xrow[(kk + 1) * 2 * G::XPITCH + xi],
                                                                wrow[(t * C1_KC + (kk + 1) * 2) * C1_TN], acc1, 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;
    acc += acc1;

    // lane holds rows (r/4)*8 + h*4 + r%4 of its wave's 32, column j
    const int co = n0 + wn * 32 + j;
    if (co >= p.Cout) return;
    const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int l = l0 + wm * 32 + (r >> 2) * 8 + h * 4 + (r & 3);
        if (l >= p.Lout) continue;
        const int ol = l * p.out_os + p.out_off;
        if (ol < 0 || ol >= p.out_L) continue;
        const size_t o = ((size_t)b * p.out_L + ol) * p.out_C + co;
        float v = acc[r] + bv;
        if (p.addend) v += p.addend[o];
        if (p.act == 1) v = nps::gelu_erf(v);
        if (p.accumulate) v += p.out[o];
        p.out[o] = v;
    }
}

__global__ void conv1d_pack_kernel(const float* __restrict__ w, float* __restrict__ wpack, int Cout, int Cin, int K,
                                   int cin_p, int cout_p) {
    const long n = (long)K * cin_p * cout_p;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % cout_p);
        const int ci = (int)((i / cout_p) % cin_p);
        const int t = (int)(i / ((long)cout_p * cin_p));
        wpack[i] = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * K + t] : 0.f;
    }
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

template <int K, int S>
int conv1d_launch(const nps_conv1d_t& p, hipStream_t s) {
    const int ltiles = (p.Lout + C1_TL - 1) / C1_TL;
    const dim3 grid((unsigned)(p.B * ltiles), (unsigned)((p.Cout + C1_TN - 1) / C1_TN));
    conv1d_kernel<K, S><<<grid, 256, 0, s>>>(p, ltiles, round_up(p.Cin, C1_KC), round_up(p.Cout, C1_TN));
    NPS_CHECK_LAUNCH("conv1d_fwd");
    return 0;
}

// ------------------------------------------------------------------------------ weight gradient
// g[m][n][t] = sum_{b,l} a[b][l][m] * xz[b][l*S + t - pad_l][n].  GEMM view: rows = a's channels, columns = x's
// channels, reduction = positions of a.  A work-group (4 waves) owns one (64 m, 64 n) tile and all K taps (a wave
// 32 x 32 with one accumulator per tap) over its share of the position tiles (64 positions of one sample).  Both
// operands are staged as they lie in memory, As[position][m] and Xs[patch position][n]: lanes read consecutive
// channels, the MFMA's k index walks positions.  Split `sp` stores its partial sums to ws[sp][t][m][n] (padded tile
// extents); wgrad1d_reduce adds the splits in order.
constexpr int W1_TP = 64;

template <int K, int S>
__global__ __launch_bounds__(256) void wgrad1d_kernel(const nps_wgrad1d_t p, int ltiles, int ntiles, int per, int n_nt,
                                                      int Mp, int Np) {
    constexpr int XP = (W1_TP - 1) * S + K;
    __shared__ __attribute__((aligned(16))) float As[W1_TP * 64];
    __shared__ __attribute__((aligned(16))) float Xs[XP * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, h = lane >> 5, j = lane & 31;
    const int nt = blockIdx.x % n_nt, mt = blockIdx.x / n_nt;
    const int m0 = mt * 64, n0 = nt * 64;
    const int t_begin = blockIdx.y * per;
    const int t_end = min(ntiles, t_begin + per);

    f32x16 acc[K];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const bool vec_a = (p.M & 3) == 0, vec_x = (p.N & 3) == 0;
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int b = tile / ltiles, l0 = (tile % ltiles) * W1_TP;
        const int f0 = l0 * S - p.pad_l;
        __syncthreads();
        for (int idx = tid; idx < W1_TP * 16; idx += 256) {
            const int pos = idx >> 4, m = m0 + (idx & 15) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int l = l0 + pos;
            if (l < p.La && m < p.M) {
                const float* row = p.a + ((size_t)b * p.La + l) * p.M;
                if (vec_a && m + 4 <= p.M) {
                    v = *reinterpret_cast<const f32x4*>(row + m);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (m + e < p.M) v[e] = row[m + e];
                }
            }
            *reinterpret_cast<f32x4*>(As + pos * 64 + (idx & 15) * 4) = v;
        }
        for (int idx = tid; idx < XP * 16; idx += 256) {
            const int pos = idx >> 4, n = n0 + (idx & 15) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int f = f0 + pos;
            if (f >= 0 && f < p.Lx && n < p.N) {
                const float* row = p.x + ((size_t)b * p.Lx + f) * p.N;
                if (vec_x && n + 4 <= p.N) {
                    v = *reinterpret_cast<const f32x4*>(row + n);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < p.N) v[e] = row[n + e];
                }
            }
            *reinterpret_cast<f32x4*>(Xs + pos * 64 + (idx & 15) * 4) = v;
        }
        __syncthreads();
        const float* ap = As + h * 64 + wm * 32 + j;
        const float* xp = Xs + (h * S) * 64 + wn * 32 + j;
#pragma unroll 4
        for (int q = 0; q < W1_TP / 2; ++q) {
            const float av = ap[q * 2 * 64];
#pragma unroll
            for (int t = 0; t < K; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xp[(q * 2 * S + t) * 64], acc[t], 0, 0, 0);
        }
    }

    const int n = n0 + wn * 32 + j;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        float* w = p.ws + ((size_t)blockIdx.y * K + t) * Mp * Np;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r >> 2) * 8 + h * 4 + (r & 3);
            w[(size_t)m * Np + n] = acc[t][r];
        }
    }
}

__global__ void wgrad1d_reduce_kernel(const float* __restrict__ ws, float* __restrict__ g, int M, int N, int K, int Mp,
                                      int Np, int splits) {
    const long total = (long)M * N * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % K);
        const int n = (int)((i / K) % N);
        const int m = (int)(i / ((long)K * N));
        float s = 0.f;
        for (int sp = 0; sp < splits; ++sp) s += ws[(((size_t)sp * K + t) * Mp + m) * Np + n];
        g[i] = s;
    }
}

struct W1Plan {
    int ltiles, ntiles, per, splits, n_mt, n_nt;
};

int wgrad1d_plan(const nps_wgrad1d_t* pp, W1Plan& pl, bool need_buffers) {
    NPS_CHECK_ARG(pp != nullptr, "conv1d_wgrad: null");
    const nps_wgrad1d_t& p = *pp;
    NPS_CHECK_ARG(p.K >= 1 && p.K <= 4, "conv1d_wgrad: K %d outside 1..4", p.K);
    NPS_CHECK_ARG(p.stride >= 1 && p.stride <= 2, "conv1d_wgrad: stride %d outside 1..2", p.stride);
    NPS_CHECK_ARG(p.B > 0 && p.La > 0 && p.M > 0 && p.Lx > 0 && p.N > 0 && p.pad_l >= 0 && p.pad_r >= 0,
                  "conv1d_wgrad: bad shape");
    NPS_CHECK_ARG(p.Lx + p.pad_l + p.pad_r >= p.K && (p.Lx + p.pad_l + p.pad_r - p.K) / p.stride + 1 == p.La,
                  "conv1d_wgrad: a's length %d is not the K=%d stride=%d conv's output over x of length %d padded by "
                  "(%d, %d)", p.La, p.K, p.stride, p.Lx, p.pad_l, p.pad_r);
    if (need_buffers) {
        NPS_CHECK_ARG(p.a && p.x && p.g && p.ws, "conv1d_wgrad: null tensor");
        NPS_CHECK_ARG(((p.M & 3) || ((uintptr_t)p.a & 15) == 0) && ((p.N & 3) || ((uintptr_t)p.x & 15) == 0) &&
                          ((uintptr_t)p.ws & 3) == 0 && ((uintptr_t)p.g & 3) == 0,
                      "conv1d_wgrad: tensors with a channel count that is a multiple of 4 must be 16-byte aligned");
    }
    pl.ltiles = (p.La + W1_TP - 1) / W1_TP;
    const long ntiles = (long)p.B * pl.ltiles;
    NPS_CHECK_ARG(ntiles < (1L << 30), "conv1d_wgrad: too many position tiles");
    pl.n_mt = (p.M + 63) / 64;
    pl.n_nt = (p.N + 63) / 64;
    const long base = (long)pl.n_mt * pl.n_nt;
    NPS_CHECK_ARG(base < (1L << 24), "conv1d_wgrad: too many channel tiles");
    // split the position tiles so that the grid puts ~4 work-groups on each of the 256 CUs, at most 64 splits; the
    // schedule depends on the shape alone
    long splits = (1024 + base - 1) / base;
    if (splits > 64) splits = 64;
    if (splits > ntiles) splits = ntiles;
    pl.per = (int)((ntiles + splits - 1) / splits);
    pl.splits = (int)((ntiles + pl.per - 1) / pl.per);
    pl.ntiles = (int)ntiles;
    return 0;
}

template <int K, int S>
int wgrad1d_launch(const nps_wgrad1d_t& p, const W1Plan& pl, hipStream_t s) {
    const int Mp = pl.n_mt * 64, Np = pl.n_nt * 64;
    const dim3 grid((unsigned)(pl.n_mt * pl.n_nt), (unsigned)pl.splits);
    wgrad1d_kernel<K, S><<<grid, 256, 0, s>>>(p, pl.ltiles, pl.ntiles, pl.per, pl.n_nt, Mp, Np);
    NPS_CHECK_LAUNCH("conv1d_wgrad");
    const long total = (long)p.M * p.N * p.K;
    const long nb = (total + 255) / 256;
    wgrad1d_reduce_kernel<<<(unsigned)(nb > 4096 ? 4096 : nb), 256, 0, s>>>(p.ws, p.g, p.M, p.N, p.K, Mp, Np,
                                                                           pl.splits);
    NPS_CHECK_LAUNCH("conv1d_wgrad reduce");
    return 0;
}

}  // namespace

// ================================================================================ C ABI
extern "C" size_t nps_conv1d_packed_floats(int Cout, int Cin, int K) {
    if (Cout <= 0 || Cin <= 0 || K < 1 || K > 4) return 0;
    return (size_t)K * round_up(Cin, C1_KC) * round_up(Cout, C1_TN);
}

extern "C" int nps_conv1d_pack_weights(const float* w, float* wpack, int Cout, int Cin, int K, void* stream) {
    NPS_CHECK_ARG(w && wpack && Cout > 0 && Cin > 0 && K >= 1 && K <= 4, "conv1d_pack_weights: bad args");
    NPS_CHECK_ARG(((uintptr_t)wpack & 15) == 0, "conv1d_pack_weights: wpack must be 16-byte aligned");
    const int cin_p = round_up(Cin, C1_KC), cout_p = round_up(Cout, C1_TN);
    const long n = (long)K * cin_p * cout_p;
    const long nb = (n + 255) / 256;
    conv1d_pack_kernel<<<(unsigned)(nb > 4096 ? 4096 : nb), 256, 0, (hipStream_t)stream>>>(w, wpack, Cout, Cin, K,
                                                                                         cin_p, cout_p);
    NPS_CHECK_LAUNCH("conv1d_pack_weights");
    return 0;
}

extern "C" int nps_conv1d_fwd(const nps_conv1d_t* pp, void* stream) {
    NPS_CHECK_ARG(pp != nullptr, "conv1d_fwd: null");
    const nps_conv1d_t& p = *pp;
    NPS_CHECK_ARG(p.K >= 1 && p.K <= 4, "conv1d_fwd: K %d outside 1..4", p.K);
    NPS_CHECK_ARG(p.stride >= 1 && p.stride <= 2, "conv1d_fwd: stride %d outside 1..2", p.stride);
    NPS_CHECK_ARG(p.nsrc >= 1 && p.nsrc <= NPS_MAX_SRC, "conv1d_fwd: nsrc %d outside 1..%d", p.nsrc, NPS_MAX_SRC);
    NPS_CHECK_ARG(p.B > 0 && p.Lc > 0 && p.Cin > 0 && p.Cout > 0 && p.pad_l >= 0 && p.pad_r >= 0, "conv1d_fwd: bad shape");
    int csum = 0;
    for (int i = 0; i < p.nsrc; ++i) {
        NPS_CHECK_ARG(p.src[i].ptr && p.src[i].C > 0 && p.src[i].L > 0 && ((uintptr_t)p.src[i].ptr & 3) == 0,
                      "conv1d_fwd: bad source %d", i);
        NPS_CHECK_ARG((long)p.B * p.src[i].L < (1L << 31), "conv1d_fwd: source %d has too many positions", i);
        csum += p.src[i].C;
    }
    NPS_CHECK_ARG(csum == p.Cin, "conv1d_fwd: the sources hold %d channels, Cin is %d", csum, p.Cin);
    NPS_CHECK_ARG(p.Lc + p.pad_l + p.pad_r >= p.K && (p.Lc + p.pad_l + p.pad_r - p.K) / p.stride + 1 == p.Lout,
                  "conv1d_fwd: Lout %d is not the K=%d stride=%d conv's output over a frame of %d padded by (%d, %d)",
                  p.Lout, p.K, p.stride, p.Lc, p.pad_l, p.pad_r);
    NPS_CHECK_ARG(p.wpack && ((uintptr_t)p.wpack & 15) == 0, "conv1d_fwd: wpack must be a 16-byte aligned packing");
    NPS_CHECK_ARG(p.out && p.out_C >= p.Cout && p.out_L > 0 && (p.out_os == 1 || p.out_os == 2),
                  "conv1d_fwd: bad output (out_C %d, Cout %d, out_L %d, out_os %d)", p.out_C, p.Cout, p.out_L, p.out_os);
    NPS_CHECK_ARG(p.out_off > -(1 << 28) && p.out_off < (1 << 28) && p.Lout < (1 << 28) && p.Lc < (1 << 28),
                  "conv1d_fwd: extent too large");
    NPS_CHECK_ARG(p.act == 0 || p.act == 1, "conv1d_fwd: act %d (0 none, 1 GELU)", p.act);
    const long ltiles = (p.Lout + C1_TL - 1) / C1_TL;
    NPS_CHECK_ARG(p.B * ltiles < (1L << 31) && (p.Cout + C1_TN - 1) / C1_TN < 65536, "conv1d_fwd: grid too large");
    hipStream_t s = (hipStream_t)stream;
    switch (p.K * 2 + p.stride - 1) {
        case 2: return conv1d_launch<1, 1>(p, s);
        case 3: return conv1d_launch<1, 2>(p, s);
        case 4: return conv1d_launch<2, 1>(p, s);
        case 5: return conv1d_launch<2, 2>(p, s);
        case 6: return conv1d_launch<3, 1>(p, s);
        case 7: return conv1d_launch<3, 2>(p, s);
        case 8: return conv1d_launch<4, 1>(p, s);
        default: return conv1d_launch<4, 2>(p, s);
    }
}

extern "C" size_t nps_conv1d_wgrad_ws_floats(const nps_wgrad1d_t* pp) {
    W1Plan pl;
    if (wgrad1d_plan(pp, pl, false) < 0) return 0;
    return (size_t)pl.splits * pp->K * (pl.n_mt * 64) * (size_t)(pl.n_nt * 64);
}

extern "C" int nps_conv1d_wgrad(const nps_wgrad1d_t* pp, void* stream) {
    W1Plan pl;
    if (wgrad1d_plan(pp, pl, true) < 0) return -1;
    const nps_wgrad1d_t& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    switch (p.K * 2 + p.stride - 1) {
        case 2: return wgrad1d_launch<1, 1>(p, pl, s);
        case 3: return wgrad1d_launch<1, 2>(p, pl, s);
        case 4: return wgrad1d_launch<2, 1>(p, pl, s);
        case 5: return wgrad1d_launch<2, 2>(p, pl, s);
        case 6: return wgrad1d_launch<3, 1>(p, pl, s);
        case 7: return wgrad1d_launch<3, 2>(p, pl, s);
        case 8: return wgrad1d_launch<4, 1>(p, pl, s);
        default: return wgrad1d_launch<4, 2>(p, pl, s);
    }
}
