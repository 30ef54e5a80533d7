// Backward (training) kernels of the 3-D U-Net convs for gfx950 (MI355X): the weight gradient of nps_conv3d
// (K^3 taps, stride 1 or 2, circular / zero frame extension) on exact fp32 MFMA, and the plain layout kernels the
// Upsample's backward needs (space-to-depth, circular pad and its adjoint fold) on NDHWC.
// Input gradients of the 3-D convs are NOT here: they are forward convs of dy with re-packed weights
// (nps_conv3d_fwd), see nps_hip/autograd.py.
#include "nps_common.hpp"

namespace {

// ------------------------------------------------------------------------------ weight gradient
// G[m][n][(kd*K + kh)*K + kw] += sum_{b, pd, ph, pw} A[b][pd][ph][pw][m] * Xext[b][pd*S + kd][ph*S + kh][pw*S + kw][n]
// GEMM view: M = A channels, N = X channels, reduction = voxels of A (split over work-groups).  The 2-D kernel's
// shape (backward.hip wgrad_kernel) one depth plane at a time: a work-group (4 waves) owns one (64 m, 64 n) tile
// and one TAP GROUP = one kd plane x RG kernel rows x K kernel columns (RG = K for K <= 3: the plane's <= 9 taps;
// RG = 2 for K = 4: 8 taps, two groups per plane — 16 accumulators of 16 registers do not fit a wave), a wave
// 32 m x 32 n with one v_mfma_f32_32x32x2_f32 accumulator per tap of the group.  Per tile of TH x TW A voxels of
// one (b, pd) slice, A is staged transposed as [m][px] (px contiguous: one ds_read_b128 feeds 4 MFMAs of every tap)
// and the X patch of depth plane pd*S + kd as [n][patch px]; A voxel (r, c) pairs with patch pixel
// (r*S + kh, c*S + kw), so stride 2 reads the input as it lies (no space-to-depth copy).
constexpr int W3_TH = 4, W3_TW = 16, W3_PX = W3_TH * W3_TW;  // 64 A voxels per tile
constexpr int W3_APITCH = W3_PX + 4;                         // 16-B aligned rows, conflict-free b128 reads

template <int K, int S>
struct W3Geo {
    static constexpr int RG = K <= 3 ? K : 2;                 // kernel rows per tap group
    static constexpr int NRG = K / RG;                        // row groups per kd plane
    static constexpr int NGRP = K * NRG;                      // tap groups per (m, n) tile
    static constexpr int TAPS = RG * K;                       // accumulators per wave (<= 9)
    static constexpr int PH = (W3_TH - 1) * S + RG, PW = (W3_TW - 1) * S + K;
    static constexpr int NP = PH * PW;                        // patch pixels
    static constexpr int BP = NP | 1;                         // odd pitch: b32 reads across n rows conflict-free
    static constexpr int NA = W3_PX * 16 / 256;               // float4 per thread: A tile
    static constexpr int NB = (NP * 16 + 255) / 256;          // float4 per thread: X patch
    static constexpr size_t LDS = sizeof(float) * (64 * W3_APITCH + 64 * BP);
};

__device__ __forceinline__ f32x4 ld4c(const float* p, int C, int c) {  // channels [c, c+4) of one voxel row
    if ((C & 3) == 0 && c + 4 <= C) return *reinterpret_cast<const f32x4*>(p + c);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < C) v[e] = p[c + e];
    return v;
}

// coordinate `e` of the extended axis (zpad zeros, circ wrapped voxels, n real ones, ...) -> real index or -1 (zero)
__device__ __forceinline__ int ext_index(int e, int n, int circ, int zpad) {
    const int v = e - zpad;
    if (v < 0 || v >= n + 2 * circ) return -1;
    return circ ? nps::wrap_mod(v - circ, n) : v;
}

template <int K, int S>
__global__ __launch_bounds__(256) void wgrad3d_kernel(const nps_wgrad3d_t p, int ntiles, int tiles_per_split, int n_nt,
                                                      int tiles_y, int tiles_x) {
    using G = W3Geo<K, S>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, h = lane >> 5;
    int r = blockIdx.x;
    const int grp = r % G::NGRP;
    r /= G::NGRP;
    const int nt = r % n_nt, mt = r / n_nt;
    const int m0 = mt * 64, n0 = nt * 64;
    const int kd = grp / G::NRG, kh0 = (grp % G::NRG) * G::RG;
    float* As = smem;                      // [64 m][W3_APITCH]
    float* Bs = smem + 64 * W3_APITCH;     // [64 n][BP]

    const int t_begin = blockIdx.y * tiles_per_split;
    const int t_end = min(ntiles, t_begin + tiles_per_split);
    if (t_begin >= t_end) return;

    // register prefetch of one tile's A (4 float4 / thread) and X patch (<= 19 float4 / thread)
    f32x4 ra[G::NA], rb[G::NB];
    auto issue = [&](int t) {
        int q = t;
        const int tx = q % tiles_x; q /= tiles_x;
        const int ty = q % tiles_y; q /= tiles_y;
        const int pd = q % p.Da, b = q / p.Da;
        const int oy0 = ty * W3_TH, ox0 = tx * W3_TW;
#pragma unroll
        for (int k = 0; k < G::NA; ++k) {
            const int idx = tid + k * 256;
            const int px = idx >> 4, mq = idx & 15;
            const int oy = oy0 + px / W3_TW, ox = ox0 + px % W3_TW;
            const int m = m0 + mq * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (oy < p.Ha && ox < p.Wa && m < p.M)
                v = ld4c(p.a + ((((size_t)b * p.Da + pd) * p.Ha + oy) * p.Wa + ox) * p.M, p.M, m);
            ra[k] = v;
        }
        const int d = ext_index(pd * S + kd, p.Dx, p.circ, p.zpad);
#pragma unroll
        for (int k = 0; k < G::NB; ++k) {
            const int idx = tid + k * 256;
            const int pp = idx >> 4, nq = idx & 15;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int n = n0 + nq * 4;
            if (pp < G::NP && d >= 0 && n < p.N) {
                const int pr = pp / G::PW, pc = pp - pr * G::PW;
                const int y = ext_index(oy0 * S + pr + kh0, p.Hx, p.circ, p.zpad);
                const int x = ext_index(ox0 * S + pc, p.Wx, p.circ, p.zpad);
                if (y >= 0 && x >= 0) v = ld4c(p.x + ((((size_t)b * p.Dx + d) * p.Hx + y) * p.Wx + x) * p.N, p.N, n);
            }
            rb[k] = v;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int k = 0; k < G::NA; ++k) {
            const int idx = tid + k * 256;
            const int px = idx >> 4, mq = idx & 15;
#pragma unroll
            for (int e = 0; e < 4; ++e) As[(mq * 4 + e) * W3_APITCH + px] = ra[k][e];
        }
#pragma unroll
        for (int k = 0; k < G::NB; ++k) {
            const int idx = tid + k * 256;
            const int pp = idx >> 4, nq = idx & 15;
            if (pp < G::NP) {
#pragma unroll
                for (int e = 0; e < 4; ++e) Bs[(nq * 4 + e) * G::BP + pp] = rb[k][e];
            }
        }
    };

    f32x16 acc[G::TAPS];
#pragma unroll
    for (int i = 0; i < G::TAPS; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    const float* arow = As + (wm * 32 + (lane & 31)) * W3_APITCH + h * 4;
    const float* brow = Bs + (wn * 32 + (lane & 31)) * G::BP;

    issue(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();
        commit();
        __syncthreads();
        if (t + 1 < t_end) issue(t + 1);
#pragma unroll
        for (int gi = 0; gi < W3_PX / 8; ++gi) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(arow + gi * 8);
            // A voxels gi*8 + h*4 + e (e < 4) lie in tile row gi/2, columns (gi&1)*8 + h*4 + e
            const float* bp0 = brow + ((gi >> 1) * S) * G::PW + ((gi & 1) * 8 + h * 4) * S;
#pragma unroll
            for (int i = 0; i < G::TAPS; ++i) {
                const float* bp = bp0 + (i / K) * G::PW + (i % K);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bp[e * S], acc[i], 0, 0, 0);
            }
        }
    }

    // accumulate this split's partial into G: lane holds rows (r/4)*8 + h*4 + r%4, column lane%32
    const int n = n0 + wn * 32 + (lane & 31);
#pragma unroll
    for (int i = 0; i < G::TAPS; ++i) {
        const int tap = (kd * K + kh0 + i / K) * K + i % K;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int m = m0 + wm * 32 + (rr >> 2) * 8 + h * 4 + (rr & 3);
            if (m < p.M && n < p.N) atomicAdd(p.g + ((size_t)m * p.N + n) * (K * K * K) + tap, acc[i][rr]);
        }
    }
}

// the launch plan: tiles of the reduction, tap groups and how many work-groups share each (m, n, group)'s voxels
struct W3Plan {
    int ntiles, per, splits, n_mt, n_nt, tiles_y, tiles_x, ngrp;
};

int wgrad3d_plan(const nps_wgrad3d_t* pp, W3Plan& pl) {
    NPS_CHECK_ARG(pp != nullptr, "conv3d_wgrad: null");
    const nps_wgrad3d_t& p = *pp;
    NPS_CHECK_ARG(p.K >= 1 && p.K <= 4, "conv3d_wgrad: K %d outside 1..4", p.K);
    NPS_CHECK_ARG(p.stride >= 1 && p.stride <= 2, "conv3d_wgrad: stride %d outside 1..2", p.stride);
    NPS_CHECK_ARG(p.a && p.x && p.g && p.B > 0 && p.Da > 0 && p.Ha > 0 && p.Wa > 0 && p.M > 0 && p.Dx > 0 && p.Hx > 0 &&
                      p.Wx > 0 && p.N > 0 && p.circ >= 0 && p.zpad >= 0,
                  "conv3d_wgrad: bad shape");
    NPS_CHECK_ARG(p.circ <= p.Dx && p.circ <= p.Hx && p.circ <= p.Wx, "conv3d_wgrad: circular extension beyond x");
    const int ext = 2 * (p.circ + p.zpad);
    NPS_CHECK_ARG(p.Dx + ext >= p.K && p.Hx + ext >= p.K && p.Wx + ext >= p.K &&
                      (p.Dx + ext - p.K) / p.stride + 1 == p.Da && (p.Hx + ext - p.K) / p.stride + 1 == p.Ha &&
                      (p.Wx + ext - p.K) / p.stride + 1 == p.Wa,
                  "conv3d_wgrad: a's extent %dx%dx%d is not the K=%d stride=%d conv's output over x %dx%dx%d "
                  "extended by circ %d + zpad %d",
                  p.Da, p.Ha, p.Wa, p.K, p.stride, p.Dx, p.Hx, p.Wx, p.circ, p.zpad);
    pl.tiles_y = (p.Ha + W3_TH - 1) / W3_TH;
    pl.tiles_x = (p.Wa + W3_TW - 1) / W3_TW;
    const long ntiles = (long)p.B * p.Da * pl.tiles_y * pl.tiles_x;
    NPS_CHECK_ARG(ntiles < (1L << 30), "conv3d_wgrad: too many tiles");
    pl.n_mt = (p.M + 63) / 64;
    pl.n_nt = (p.N + 63) / 64;
    pl.ngrp = p.K <= 3 ? p.K : p.K * (p.K / 2);
    const long base = (long)pl.n_mt * pl.n_nt * pl.ngrp;
    // split the voxel tiles so the grid puts ~4 work-groups on each of the 256 CUs, >= 8 tiles each
    long splits = (1024 + base - 1) / base;
    const long max_splits = (ntiles + 7) / 8;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    pl.per = (int)((ntiles + splits - 1) / splits);
    splits = (ntiles + pl.per - 1) / pl.per;
    NPS_CHECK_ARG(base < (1L << 31) && splits < 65536, "conv3d_wgrad: grid too large");
    pl.ntiles = (int)ntiles;
    pl.splits = (int)splits;
    return 0;
}

template <int K, int S>
int wgrad3d_launch(const nps_wgrad3d_t& p, const W3Plan& pl, hipStream_t s) {
    using G = W3Geo<K, S>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)wgrad3d_kernel<K, S>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)G::LDS);
        attr_set = true;
    }
    const dim3 grid((unsigned)(pl.n_mt * pl.n_nt * pl.ngrp), (unsigned)pl.splits);
    wgrad3d_kernel<K, S><<<grid, 256, G::LDS, s>>>(p, pl.ntiles, pl.per, pl.n_nt, pl.tiles_y, pl.tiles_x);
    NPS_CHECK_LAUNCH("conv3d_wgrad");
    return 0;
}

// ------------------------------------------------------------------------------ layout helpers (NDHWC fp32)
// out[b][q][(rd, rh, rw, c)] = x[b][2 q + r][c] (0 outside x): the K = 4 / stride-2 conv of the Upsample's backward
// becomes a K = 2 / stride-1 conv over 8 C channels
__global__ void space_to_depth3d_kernel(const float* __restrict__ x, float* __restrict__ out, int D, int H, int W, int C,
                                        int Dq, int Hq, int Wq) {
    const int b = blockIdx.y;
    const long n = (long)Dq * Hq * Wq * 8 * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % (8 * C));
        long vox = i / (8 * C);
        const int par = cc / C, c = cc - par * C;
        const int wq = (int)(vox % Wq); vox /= Wq;
        const int hq = (int)(vox % Hq);
        const int dq = (int)(vox / Hq);
        const int d = 2 * dq + (par >> 2), hh = 2 * hq + ((par >> 1) & 1), w = 2 * wq + (par & 1);
        out[(size_t)b * n + i] =
            (d < D && hh < H && w < W) ? x[((((size_t)b * D + d) * H + hh) * W + w) * C + c] : 0.f;
    }
}

// out[b][Z][Y][X][c] = x[b][(Z - pad) mod D][(Y - pad) mod H][(X - pad) mod W][c]
__global__ void circ_pad3d_kernel(const float* __restrict__ x, float* __restrict__ out, int D, int H, int W, int C,
                                  int pad) {
    const int b = blockIdx.y;
    const int Do = D + 2 * pad, Ho = H + 2 * pad, Wo = W + 2 * pad;
    const long n = (long)Do * Ho * Wo * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long vox = i / C;
        const int X = (int)(vox % Wo); vox /= Wo;
        const int Y = (int)(vox % Ho);
        const int Z = (int)(vox / Ho);
        const int z = nps::wrap_mod(Z - pad, D), y = nps::wrap_mod(Y - pad, H), xx = nps::wrap_mod(X - pad, W);
        out[(size_t)b * n + i] = x[((((size_t)b * D + z) * H + y) * W + xx) * C + c];
    }
}

// adjoint of circ_pad3d: gx[b][z][y][x][c] = sum of gp over the padded positions that wrap to (z, y, x)
__global__ void circ_fold3d_kernel(const float* __restrict__ gp, float* __restrict__ gx, int D, int H, int W, int C,
                                   int pad) {
    const int b = blockIdx.y;
    const int Dp = D + 2 * pad, Hp = H + 2 * pad, Wp = W + 2 * pad;
    const long n = (long)D * H * W * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long vox = i / C;
        const int x = (int)(vox % W); vox /= W;
        const int y = (int)(vox % H);
        const int z = (int)(vox / H);
        float s = 0.f;
        for (int Z = (z + pad) % D; Z < Dp; Z += D)          // smallest Z >= 0 with Z = z + pad (mod D)
            for (int Y = (y + pad) % H; Y < Hp; Y += H)
                for (int X = (x + pad) % W; X < Wp; X += W)
                    s += gp[((((size_t)b * Dp + Z) * Hp + Y) * Wp + X) * C + c];
        gx[(size_t)b * n + i] = s;
    }
}

inline unsigned blocks_for(long n) {
    const long nb = (n + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb > 4096 ? 4096 : nb);
}

}  // namespace

// ================================================================================ C ABI
extern "C" int nps_conv3d_wgrad_splits(const nps_wgrad3d_t* pp) {
    W3Plan pl;
    if (wgrad3d_plan(pp, pl) < 0) return -1;
    return pl.splits;
}

extern "C" int nps_conv3d_wgrad(const nps_wgrad3d_t* pp, void* stream) {
    W3Plan pl;
    if (wgrad3d_plan(pp, pl) < 0) return -1;
    const nps_wgrad3d_t& p = *pp;
    hipStream_t s = (hipStream_t)stream;
    switch (p.K * 2 + p.stride - 1) {
        case 2: return wgrad3d_launch<1, 1>(p, pl, s);
        case 3: return wgrad3d_launch<1, 2>(p, pl, s);
        case 4: return wgrad3d_launch<2, 1>(p, pl, s);
        case 5: return wgrad3d_launch<2, 2>(p, pl, s);
        case 6: return wgrad3d_launch<3, 1>(p, pl, s);
        case 7: return wgrad3d_launch<3, 2>(p, pl, s);
        case 8: return wgrad3d_launch<4, 1>(p, pl, s);
        default: return wgrad3d_launch<4, 2>(p, pl, s);
    }
}

extern "C" int nps_space_to_depth3d(const float* x, float* out, int B, int D, int H, int W, int C, int Dq, int Hq,
                                    int Wq, void* stream) {
    NPS_CHECK_ARG(x && out && B > 0 && B < 65536 && D > 0 && H > 0 && W > 0 && C > 0 && Dq > 0 && Hq > 0 && Wq > 0,
                  "space_to_depth3d: bad args");
    const long n = (long)Dq * Hq * Wq * 8 * C;
    space_to_depth3d_kernel<<<dim3(blocks_for(n), (unsigned)B), 256, 0, (hipStream_t)stream>>>(x, out, D, H, W, C, Dq,
                                                                                           Hq, Wq);
    NPS_CHECK_LAUNCH("space_to_depth3d");
    return 0;
}

extern "C" int nps_circular_pad3d(const float* x, float* out, int B, int D, int H, int W, int C, int pad,
                                  void* stream) {
    NPS_CHECK_ARG(x && out && B > 0 && B < 65536 && D > 0 && H > 0 && W > 0 && C > 0 && pad >= 0,
                  "circular_pad3d: bad args");
    const long n = (long)(D + 2 * pad) * (H + 2 * pad) * (W + 2 * pad) * C;
    circ_pad3d_kernel<<<dim3(blocks_for(n), (unsigned)B), 256, 0, (hipStream_t)stream>>>(x, out, D, H, W, C, pad);
    NPS_CHECK_LAUNCH("circular_pad3d");
    return 0;
}

extern "C" int nps_circular_fold3d(const float* gp, float* gx, int B, int D, int H, int W, int C, int pad,
                                   void* stream) {
    NPS_CHECK_ARG(gp && gx && B > 0 && B < 65536 && D > 0 && H > 0 && W > 0 && C > 0 && pad >= 0,
                  "circular_fold3d: bad args");
    const long n = (long)D * H * W * C;
    circ_fold3d_kernel<<<dim3(blocks_for(n), (unsigned)B), 256, 0, (hipStream_t)stream>>>(gp, gx, D, H, W, C, pad);
    NPS_CHECK_LAUNCH("circular_fold3d");
    return 0;
}
