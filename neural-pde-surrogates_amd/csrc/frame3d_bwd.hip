// The 3-D frame of the differentiable U-Net walk on NDHWC fp32 (gfx950): act(GroupNorm(cat(crop_Nd(src_i)))) with
// exactly Cin channels (nps_frame3d_fwd), its backward (nps_frame3d_bwd, the 3-D form of nps_frame_pack_bwd2 — the
// maths is in the comment above frame_bwd_reduce_kernel in backward.hip) and the residual add at a crop offset
// (nps_add_at_copy3d).  The 2-D kernels cannot serve the (B, D*H, W, C) view once a source has an offset along D
// or H.  Every kernel streams its tensors once: thread = one fixed channel unit (a quad with 16-B accesses when
// every channel count is a multiple of 4, else one channel) x a strided share of the work-group's voxels, sums in
// registers (measured rates: profiles/unet3d_train/README.md).  All voxel <-> voxel mappings go through the three
// __host__ __device__ functions below, which nps_frame3d_locate exposes to the CPU tests.
#include "nps_common.hpp"
#include <algorithm>

namespace {

constexpr int F3_U = 4;  // voxels per loop step: their loads issue before the first use

struct Vox {
    int d, h, w;
};

// linear voxel index of a [D][H][W] volume -> (d, h, w)
__host__ __device__ inline Vox f3_split(int v, int H, int W) {
    Vox r;
    r.d = v / (H * W);
    const int rem = v - r.d * (H * W);
    r.h = rem / W;
    r.w = rem - r.h * W;
    return r;
}

// frame voxel f -> linear index of the voxel of source S placed on it, or -1 where S does not cover f
__host__ __device__ inline int f3_src_index(const nps_src3_t& S, Vox f) {
    const int d = f.d - S.off_d, h = f.h - S.off_h, w = f.w - S.off_w;
    if (d < 0 || d >= S.D || h < 0 || h >= S.H || w < 0 || w >= S.W) return -1;
    return (d * S.H + h) * S.W + w;
}

// voxel s of source S -> linear index of the frame voxel it lands on, or -1 where it lies outside the frame
__host__ __device__ inline int f3_frame_index(const nps_src3_t& S, int Dc, int Hc, int Wc, Vox s) {
    const int d = s.d + S.off_d, h = s.h + S.off_h, w = s.w + S.off_w;
    if (d < 0 || d >= Dc || h < 0 || h >= Hc || w < 0 || w >= Wc) return -1;
    return (d * Hc + h) * Wc + w;
}

template <int V>
struct Pack {
    float v[V];
};

template <int V>
__device__ __forceinline__ Pack<V> f3_zero() {
    Pack<V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = 0.f;
    return r;
}

template <int V>
__device__ __forceinline__ Pack<V> f3_ld(const float* p) {
    Pack<V> r;
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) r.v[e] = t[e];
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int V>
__device__ __forceinline__ void f3_st(float* p, const Pack<V>& x) {
    if constexpr (V == 4)
        *reinterpret_cast<f32x4*>(p) = f32x4{x.v[0], x.v[1], x.v[2], x.v[3]};
    else
        *p = x.v[0];
}

__device__ __forceinline__ nps_src3_t f3_src(const nps_conv3d_t& a, int si) {  // (selects: no indexed kernarg copy)
    return si == 0 ? a.src[0] : (si == 1 ? a.src[1] : a.src[2]);
}

struct F3Unit {  // the source that holds frame channel c0, and c0's channel inside it
    nps_src3_t S;
    int cs;
};
__device__ __forceinline__ F3Unit f3_unit(const nps_conv3d_t& a, int c0) {
    const int C0 = a.src[0].C, C1 = a.nsrc > 1 ? a.src[1].C : 0;
    F3Unit u;
    const int si = c0 < C0 ? 0 : (c0 < C0 + C1 ? 1 : 2);
    u.S = f3_src(a, si);
    u.cs = c0 - (si == 0 ? 0 : (si == 1 ? C0 : C0 + C1));
    return u;
}

// (mean, rstd) of sample b's GroupNorm groups from the frame's fp64 moments
__device__ __forceinline__ void f3_tab_fill(const nps_conv3d_t& a, int b, float2* tab) {
    if (a.gn_stats != nullptr && (int)threadIdx.x < a.gn_groups) {
        const double cnt = (double)(a.Cin / a.gn_groups) * a.Dc * a.Hc * a.Wc;
        const double s1 = a.gn_stats[(b * a.gn_groups + threadIdx.x) * 2];
        const double s2 = a.gn_stats[(b * a.gn_groups + threadIdx.x) * 2 + 1];
        const double mean = s1 / cnt;
        double var = s2 / cnt - mean * mean;
        var = var < 0.0 ? 0.0 : var;
        tab[threadIdx.x] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)a.gn_eps)));
    }
}

// GroupNorm operands of the channel unit at c0
template <int V>
struct F3Norm {
    Pack<V> gam, bet;
    float2 mr;
};
template <int V>
__device__ __forceinline__ F3Norm<V> f3_norm(const nps_conv3d_t& a, int c0, const float2* tab, int cpg) {
    F3Norm<V> n;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        n.gam.v[e] = 1.f;
        n.bet.v[e] = 0.f;
    }
    n.mr = make_float2(0.f, 1.f);
    if (a.gn_stats != nullptr) {
        n.gam = f3_ld<V>(a.gn_gamma + c0);
        n.bet = f3_ld<V>(a.gn_beta + c0);
        n.mr = tab[c0 / cpg];
    }
    return n;
}

// The work-group's thread layout over U channel units: U <= 256: unit tid % U of voxel lane tid / U (`per` lanes);
// more units: one lane, every thread walks units tid, tid + 256, ...
struct F3Lanes {
    int per, lr, u0;
};
__device__ __forceinline__ F3Lanes f3_lanes(int U) {
    F3Lanes l;
    if (U <= 256) {
        l.per = 256 / U;
        l.lr = (int)threadIdx.x / U;
        l.u0 = (int)threadIdx.x - l.lr * U;
    } else {
        l.per = 1;
        l.lr = 0;
        l.u0 = (int)threadIdx.x;
    }
    return l;
}

// out[b][vox][c] = act(GN(frame value)), thread = one channel unit of one frame voxel
template <int V>
__global__ __launch_bounds__(256) void frame3d_fwd_kernel(const nps_conv3d_t a, float* __restrict__ out) {
    __shared__ float2 tab[16];
    const int b = blockIdx.y;
    f3_tab_fill(a, b, tab);
    __syncthreads();
    const int U = a.Cin / V, cpg = a.gn_stats ? a.Cin / a.gn_groups : 1;
    const int nvox = a.Dc * a.Hc * a.Wc;
    const long n = (long)nvox * U;
    float* ob = out + (size_t)b * nvox * a.Cin;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int vox = (int)(i / U), c0 = (int)(i - (long)vox * U) * V;
        const F3Unit u = f3_unit(a, c0);
        const int si = f3_src_index(u.S, f3_split(vox, a.Hc, a.Wc));
        Pack<V> x = f3_zero<V>();
        if (si >= 0)
            x = f3_ld<V>(reinterpret_cast<const float*>(u.S.ptr) +
                         ((size_t)b * u.S.D * u.S.H * u.S.W + si) * u.S.C + u.cs);
        const F3Norm<V> nm = f3_norm<V>(a, c0, tab, cpg);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float z = x.v[e];
            if (a.gn_stats) z = (z - nm.mr.x) * nm.mr.y * nm.gam.v[e] + nm.bet.v[e];
            x.v[e] = a.pre_act == 1 ? nps::gelu_erf(z) : z;
        }
        f3_st<V>(ob + (size_t)vox * a.Cin + c0, x);
    }
}

// Pass 1 (GroupNorm frames only): PQ[b][0][c] += sum_vox gz, PQ[b][1][c] += sum_vox gz * xhat over the work-group's
// vpb frame voxels; per-thread sums in registers, one LDS add per channel per thread, then one fp64 atomic pair
// per channel per work-group.
template <int V>
__global__ __launch_bounds__(256) void frame3d_bwd_reduce_kernel(const nps_conv3d_t a, const float* __restrict__ gy,
                                                                 double* __restrict__ PQ, int vpb) {
    extern __shared__ float part[];  // [2][Cin]
    __shared__ float2 tab[16];
    const int b = blockIdx.y;
    f3_tab_fill(a, b, tab);
    for (int c = threadIdx.x; c < 2 * a.Cin; c += blockDim.x) part[c] = 0.f;
    __syncthreads();
    const int U = a.Cin / V, cpg = a.Cin / a.gn_groups;
    const F3Lanes l = f3_lanes(U);
    const int nvox = a.Dc * a.Hc * a.Wc;
    const int p0 = blockIdx.x * vpb, p1 = min(nvox, p0 + vpb);
    if (l.lr < l.per)
        for (int u = l.u0; u < U; u += 256) {
            const int c0 = u * V;
            const F3Unit un = f3_unit(a, c0);
            const F3Norm<V> nm = f3_norm<V>(a, c0, tab, cpg);
            const float* sb =
                reinterpret_cast<const float*>(un.S.ptr) + (size_t)b * un.S.D * un.S.H * un.S.W * un.S.C + un.cs;
            const float* g = gy + (size_t)b * nvox * a.Cin + c0;
            float P[V], Q[V];
#pragma unroll
            for (int e = 0; e < V; ++e) P[e] = Q[e] = 0.f;
            for (int vox = p0 + l.lr; vox < p1; vox += F3_U * l.per) {
                Pack<V> v[F3_U], gz[F3_U];
#pragma unroll
                for (int k = 0; k < F3_U; ++k) {
                    const int vk = vox + k * l.per;
                    v[k] = f3_zero<V>();
                    gz[k] = f3_zero<V>();
                    if (vk < p1) {
                        const int si = f3_src_index(un.S, f3_split(vk, a.Hc, a.Wc));
                        if (si >= 0) v[k] = f3_ld<V>(sb + (size_t)si * un.S.C);
                        gz[k] = f3_ld<V>(g + (size_t)vk * a.Cin);
                    }
                }
#pragma unroll
                for (int k = 0; k < F3_U; ++k)
#pragma unroll
                    for (int e = 0; e < V; ++e) {  // (a voxel past p1 has gz = 0: adds nothing)
                        const float xh = (v[k].v[e] - nm.mr.x) * nm.mr.y;
                        float gk = gz[k].v[e];
                        if (a.pre_act == 1) gk *= nps::gelu_erf_grad(xh * nm.gam.v[e] + nm.bet.v[e]);
                        P[e] += gk;
                        Q[e] = fmaf(gk, xh, Q[e]);
                    }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                atomicAdd(&part[c0 + e], P[e]);
                atomicAdd(&part[a.Cin + c0 + e], Q[e]);
            }
        }
    __syncthreads();
    for (int c = threadIdx.x; c < a.Cin; c += blockDim.x) {
        atomicAdd(&PQ[(size_t)(b * 2) * a.Cin + c], (double)part[c]);
        atomicAdd(&PQ[(size_t)(b * 2 + 1) * a.Cin + c], (double)part[a.Cin + c]);
    }
}

// s12[g] = (sum over group g's channels of gamma[c] * (P, Q)[b][c]) / N: wave w takes groups w, w + 4, ..., its lanes
// a strided share of the group's channels.  The caller barriers before reading s12.
__device__ __forceinline__ void f3_s12(const nps_conv3d_t& a, const double* __restrict__ PQ, int b, int cpg,
                                       float (*s12)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* P = PQ + (size_t)(b * 2) * a.Cin;
    const double* Q = P + a.Cin;
    const double N = (double)cpg * a.Dc * a.Hc * a.Wc;
    for (int g = wave; g < a.gn_groups; g += 4) {
        double s1 = 0.0, s2 = 0.0;
        for (int c = g * cpg + lane; c < (g + 1) * cpg; c += 64) {
            const double ga = (double)a.gn_gamma[c];
            s1 += ga * P[c];
            s2 += ga * Q[c];
        }
        s1 = nps::wave_sum(s1);
        s2 = nps::wave_sum(s2);
        if (lane == 0) {
            s12[g][0] = (float)(s1 / N);
            s12[g][1] = (float)(s2 / N);
        }
    }
}

// Pass 2: dgamma / dbeta (one work-group) and, for source blockIdx.z, dx at every voxel of the source: the frame's
// gradient where the voxel lands inside the frame, exactly 0 elsewhere.
template <int V>
__global__ __launch_bounds__(256) void frame3d_bwd_apply_kernel(const nps_conv3d_t a, const float* __restrict__ gy,
                                                                const double* __restrict__ PQ, float* d0, float* d1,
                                                                float* d2, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta,
                                                                const float* __restrict__ gy2, int vpb) {
    __shared__ float2 tab[16];
    __shared__ float s12[16][2];
    const int b = blockIdx.y, si = blockIdx.z;
    const bool gn = a.gn_stats != nullptr;
    f3_tab_fill(a, b, tab);
    const int cpg = gn ? a.Cin / a.gn_groups : 1;
    if (gn) f3_s12(a, PQ, b, cpg, s12);
    if (gn && b == 0 && si == 0 && blockIdx.x == 0 && dgamma) {
        for (int c = threadIdx.x; c < a.Cin; c += blockDim.x) {
            double sg = 0.0, sb = 0.0;
            for (int bb = 0; bb < a.B; ++bb) {
                sb += PQ[(size_t)(bb * 2) * a.Cin + c];
                sg += PQ[(size_t)(bb * 2 + 1) * a.Cin + c];
            }
            dgamma[c] = (float)sg;
            dbeta[c] = (float)sb;
        }
    }
    __syncthreads();
    float* dst = si == 0 ? d0 : (si == 1 ? d1 : d2);
    if (dst == nullptr) return;
    const nps_src3_t S = f3_src(a, si);
    const int lo = si == 0 ? 0 : (si == 1 ? a.src[0].C : a.src[0].C + a.src[1].C);
    const int U = S.C / V;
    const F3Lanes l = f3_lanes(U);
    const int ns = S.D * S.H * S.W, nvox = a.Dc * a.Hc * a.Wc;
    const int p0 = blockIdx.x * vpb, p1 = min(ns, p0 + vpb);
    if (l.lr >= l.per) return;
    for (int u = l.u0; u < U; u += 256) {
        const int c0 = lo + u * V;
        const F3Norm<V> nm = f3_norm<V>(a, c0, tab, cpg);
        const float t1 = gn ? s12[c0 / cpg][0] : 0.f, t2 = gn ? s12[c0 / cpg][1] : 0.f;
        const float* sp = reinterpret_cast<const float*>(S.ptr) + (size_t)b * ns * S.C + u * V;
        float* dp = dst + (size_t)b * ns * S.C + u * V;
        const float* g = gy + (size_t)b * nvox * a.Cin + c0;
        // gy2 (or NULL): the gradient of the plain concatenation from its second consumer, added in this pass
        const float* g2 = gy2 != nullptr ? gy2 + (size_t)b * nvox * a.Cin + c0 : nullptr;
        for (int vox = p0 + l.lr; vox < p1; vox += F3_U * l.per) {
            Pack<V> v[F3_U], gz[F3_U], gp[F3_U];
            bool in[F3_U];
#pragma unroll
            for (int k = 0; k < F3_U; ++k) {
                const int vk = vox + k * l.per;
                v[k] = f3_zero<V>();
                gz[k] = f3_zero<V>();
                gp[k] = f3_zero<V>();
                in[k] = false;
                if (vk < p1) {
                    const int fi = f3_frame_index(S, a.Dc, a.Hc, a.Wc, f3_split(vk, S.H, S.W));
                    in[k] = fi >= 0;
                    if (in[k]) {
                        v[k] = f3_ld<V>(sp + (size_t)vk * S.C);
                        gz[k] = f3_ld<V>(g + (size_t)fi * a.Cin);
                        if (g2 != nullptr) gp[k] = f3_ld<V>(g2 + (size_t)fi * a.Cin);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < F3_U; ++k) {
                const int vk = vox + k * l.per;
                if (vk >= p1) break;
                Pack<V> d = f3_zero<V>();
                if (in[k]) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        float gk = gz[k].v[e];
                        if (gn) {
                            const float xh = (v[k].v[e] - nm.mr.x) * nm.mr.y;
                            if (a.pre_act == 1) gk *= nps::gelu_erf_grad(xh * nm.gam.v[e] + nm.bet.v[e]);
                            d.v[e] = nm.mr.y * (nm.gam.v[e] * gk - t1 - xh * t2);
                        } else {
                            if (a.pre_act == 1) gk *= nps::gelu_erf_grad(v[k].v[e]);
                            d.v[e] = gk;
                        }
                        d.v[e] += gp[k].v[e];
                    }
                }
                f3_st<V>(dp + (size_t)vk * S.C, d);
            }
        }
    }
}

// out = base + crop_Nd(src) placed at S's offsets, thread = one channel unit of one voxel of out
template <int V>
__global__ __launch_bounds__(256) void add_at_copy3d_kernel(float* __restrict__ out, const float* __restrict__ base,
                                                            const nps_src3_t S, int Do, int Ho, int Wo) {
    const int b = blockIdx.y;
    const int U = S.C / V;
    const int nvox = Do * Ho * Wo;
    const long n = (long)nvox * U;
    const float* bb = base + (size_t)b * nvox * S.C;
    float* ob = out + (size_t)b * nvox * S.C;
    const float* sb = reinterpret_cast<const float*>(S.ptr) + (size_t)b * S.D * S.H * S.W * S.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int vox = (int)(i / U), c0 = (int)(i - (long)vox * U) * V;
        Pack<V> x = f3_ld<V>(bb + (size_t)vox * S.C + c0);
        const int si = f3_src_index(S, f3_split(vox, Ho, Wo));
        if (si >= 0) {
            const Pack<V> s = f3_ld<V>(sb + (size_t)si * S.C + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) x.v[e] += s.v[e];
        }
        f3_st<V>(ob + (size_t)vox * S.C + c0, x);
    }
}

inline unsigned f3_grid(long n, int per_block, int cap) {
    const long nb = (n + per_block - 1) / per_block;
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

inline bool f3_aligned(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// the frame description shared by nps_frame3d_fwd / _bwd / _locate (host only; pointers only compared with NULL)
int f3_check(const nps_conv3d_t& a, const char* who) {
    NPS_CHECK_ARG(a.bf16 == 0, "%s: fp32 only (bf16 frames are not differentiated)", who);
    NPS_CHECK_ARG(a.nsrc >= 1 && a.nsrc <= NPS_MAX_SRC && a.B > 0 && a.B <= 65535 && a.Dc > 0 && a.Hc > 0 &&
                      a.Wc > 0 && a.Cin > 0,
                  "%s: bad frame (nsrc %d)", who, a.nsrc);
    NPS_CHECK_ARG((long)a.Dc * a.Hc * a.Wc < (1L << 30), "%s: frame too large", who);
    int cs = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        const nps_src3_t& s = a.src[i];
        NPS_CHECK_ARG(s.ptr != nullptr && s.C > 0 && s.D > 0 && s.H > 0 && s.W > 0, "%s: bad source %d", who, i);
        NPS_CHECK_ARG((long)s.D * s.H * s.W < (1L << 30), "%s: source %d too large", who, i);
        cs += s.C;
    }
    NPS_CHECK_ARG(cs == a.Cin, "%s: sources hold %d channels, frame Cin %d", who, cs, a.Cin);
    NPS_CHECK_ARG(a.gn_stats == nullptr || (a.gn_groups >= 1 && a.gn_groups <= 16 && a.Cin % a.gn_groups == 0 &&
                                            a.gn_gamma != nullptr && a.gn_beta != nullptr),
                  "%s: bad GroupNorm (groups %d must divide Cin %d, <= 16)", who, a.gn_groups, a.Cin);
    NPS_CHECK_ARG(a.pre_act == 0 || a.pre_act == 1, "%s: pre_act 0 or 1", who);
    NPS_CHECK_ARG(a.Cin <= 4096, "%s: Cin too large", who);
    return 0;
}

// quad kernels: every source's C (so Cin) and the GroupNorm group size multiples of 4, 16-B aligned sources
bool f3_quad(const nps_conv3d_t& a) {
    bool quad = !a.gn_stats || ((a.Cin / a.gn_groups) & 3) == 0;
    for (int i = 0; i < a.nsrc; ++i) quad = quad && (a.src[i].C & 3) == 0 && f3_aligned(a.src[i].ptr);
    return quad && (!a.gn_stats || (f3_aligned(a.gn_gamma) && f3_aligned(a.gn_beta)));
}

}  // namespace

// ================================================================================ C ABI
extern "C" int nps_frame3d_locate(const nps_conv3d_t* ap, int si, int d, int h, int w, int* fd, int* fh, int* fw) {
    NPS_CHECK_ARG(ap != nullptr && fd && fh && fw, "frame3d_locate: null");
    const nps_conv3d_t& a = *ap;
    if (f3_check(a, "frame3d_locate") < 0) return -1;
    NPS_CHECK_ARG(si >= 0 && si < a.nsrc, "frame3d_locate: source %d of %d", si, a.nsrc);
    const nps_src3_t& S = a.src[si];
    NPS_CHECK_ARG(d >= 0 && d < S.D && h >= 0 && h < S.H && w >= 0 && w < S.W, "frame3d_locate: voxel outside source");
    const int lin = (d * S.H + h) * S.W + w;
    const Vox s = f3_split(lin, S.H, S.W);
    NPS_CHECK_ARG(s.d == d && s.h == h && s.w == w, "frame3d_locate: split(%d) = (%d, %d, %d)", lin, s.d, s.h, s.w);
    const int fi = f3_frame_index(S, a.Dc, a.Hc, a.Wc, s);
    if (fi < 0) return 0;
    const Vox f = f3_split(fi, a.Hc, a.Wc);
    // the forward's direction (frame voxel -> source voxel) must land back on the same voxel
    NPS_CHECK_ARG(f3_src_index(S, f) == lin, "frame3d_locate: frame voxel %d does not map back to source voxel %d", fi,
                  lin);
    *fd = f.d;
    *fh = f.h;
    *fw = f.w;
    return 1;
}

extern "C" int nps_frame3d_fwd(const nps_conv3d_t* ap, float* out, void* stream) {
    NPS_CHECK_ARG(ap != nullptr && out != nullptr, "frame3d_fwd: null");
    const nps_conv3d_t& a = *ap;
    if (f3_check(a, "frame3d_fwd") < 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const long nvox = (long)a.Dc * a.Hc * a.Wc;
    if (f3_quad(a) && f3_aligned(out))
        frame3d_fwd_kernel<4><<<dim3(f3_grid(nvox * (a.Cin / 4), 256 * 4, 4096), a.B), 256, 0, s>>>(a, out);
    else
        frame3d_fwd_kernel<1><<<dim3(f3_grid(nvox * a.Cin, 256 * 8, 4096), a.B), 256, 0, s>>>(a, out);
    NPS_CHECK_LAUNCH("frame3d_fwd");
    return 0;
}

extern "C" int nps_frame3d_bwd(const nps_conv3d_t* ap, const float* gy, const float* gy_plain, float* const* dsrc,
                               float* dgamma, float* dbeta, double* work, void* stream) {
    NPS_CHECK_ARG(ap != nullptr && gy != nullptr && dsrc != nullptr, "frame3d_bwd: null");
    const nps_conv3d_t& a = *ap;
    if (f3_check(a, "frame3d_bwd") < 0) return -1;
    NPS_CHECK_ARG(!a.gn_stats || work != nullptr, "frame3d_bwd: GroupNorm needs work");
    hipStream_t s = (hipStream_t)stream;
    float* d[3] = {dsrc[0], a.nsrc > 1 ? dsrc[1] : nullptr, a.nsrc > 2 ? dsrc[2] : nullptr};
    bool quad = f3_quad(a) && f3_aligned(gy) && f3_aligned(gy_plain);
    for (int i = 0; i < 3; ++i) quad = quad && f3_aligned(d[i]);
    const int nvox = a.Dc * a.Hc * a.Wc;
    int smax = 1;
    for (int i = 0; i < a.nsrc; ++i) smax = std::max(smax, a.src[i].D * a.src[i].H * a.src[i].W);
    // voxels per work-group: 256, halved (down to 64) while the grid has < ~4 work-groups per CU
    int vpb = 256;
    while (vpb > 64 && (long)((std::max(nvox, smax) + vpb - 1) / vpb) * a.B < 1000) vpb >>= 1;
    if (a.gn_stats) {
        const dim3 grid((nvox + vpb - 1) / vpb, a.B);
        const size_t lds = sizeof(float) * 2 * a.Cin;
        if (quad)
            frame3d_bwd_reduce_kernel<4><<<grid, 256, lds, s>>>(a, gy, work, vpb);
        else
            frame3d_bwd_reduce_kernel<1><<<grid, 256, lds, s>>>(a, gy, work, vpb);
        NPS_CHECK_LAUNCH("frame3d_bwd reduce");
    }
    const dim3 grid((smax + vpb - 1) / vpb, a.B, a.nsrc);
    if (quad)
        frame3d_bwd_apply_kernel<4><<<grid, 256, 0, s>>>(a, gy, work, d[0], d[1], d[2], dgamma, dbeta, gy_plain, vpb);
    else
        frame3d_bwd_apply_kernel<1><<<grid, 256, 0, s>>>(a, gy, work, d[0], d[1], d[2], dgamma, dbeta, gy_plain, vpb);
    NPS_CHECK_LAUNCH("frame3d_bwd apply");
    return 0;
}

extern "C" int nps_add_at_copy3d(float* out, const float* base, const float* src, int B, int Do, int Ho, int Wo, int Ds,
                                 int Hs, int Ws, int C, int off_d, int off_h, int off_w, void* stream) {
    NPS_CHECK_ARG(out && base && src && B > 0 && B <= 65535 && Do > 0 && Ho > 0 && Wo > 0 && Ds > 0 && Hs > 0 &&
                      Ws > 0 && C > 0,
                  "add_at_copy3d: bad args");
    NPS_CHECK_ARG((long)Do * Ho * Wo < (1L << 30) && (long)Ds * Hs * Ws < (1L << 30), "add_at_copy3d: volume too large");
    nps_src3_t S;
    S.ptr = src;
    S.C = C;
    S.D = Ds;
    S.H = Hs;
    S.W = Ws;
    S.off_d = off_d;
    S.off_h = off_h;
    S.off_w = off_w;
    const long nvox = (long)Do * Ho * Wo;
    hipStream_t s = (hipStream_t)stream;
    if ((C & 3) == 0 && f3_aligned(out) && f3_aligned(base) && f3_aligned(src))
        add_at_copy3d_kernel<4><<<dim3(f3_grid(nvox * (C / 4), 256 * 4, 4096), B), 256, 0, s>>>(out, base, S, Do, Ho, Wo);
    else
        add_at_copy3d_kernel<1><<<dim3(f3_grid(nvox * C, 256 * 8, 4096), B), 256, 0, s>>>(out, base, S, Do, Ho, Wo);
    NPS_CHECK_LAUNCH("add_at_copy3d");
    return 0;
}
