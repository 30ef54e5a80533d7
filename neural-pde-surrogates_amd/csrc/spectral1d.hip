// SpectralConv1d for gfx950 (proc_fno.py:158-222): truncated DFT analysis along L, the shared per-mode complex
// mixer (spectral.hip, R = 1), truncated inverse DFT + c2r synthesis, FiLM on the mixed modes, and the one-call
// composites (include/nps.h "SpectralConv1d").  Activations are channels-last (B, L, C).
//
// A 1-D signal has no H axis to draw a grid from, so both transforms split L:
//  * analysis: work-group = (batch, 64 / 128 channels, a run of L); a thread owns one 4-channel quad x MK modes and
//    walks its sub-chunk of L.  The work-group adds its sub-chunks in ascending order through LDS and writes one
//    partial spectrum; a second kernel sums the partials of one (b, k, c) in ascending work-group order (no
//    atomics: the same inputs give the same bits).
//  * synthesis: work-group = (batch, 64 / 128 channels, a run of L) with that group's whole Z [m][CG] staged in LDS;
//    a thread owns one 4-channel quad x 8 points and walks the modes.  No cross-work-group reduction.
// Twiddles are sincospif of the exact integer phase (k l mod L) / L, built per point tile in LDS.  All arithmetic
// is fp32 fmaf chains.
#include "nps_common.hpp"

#include <climits>

namespace {

constexpr int MAX_M = 128;      // retained modes
constexpr int MAX_L = 65536;    // grid points
constexpr int PT = 16;          // points per twiddle tile of one analysis slot
constexpr int XB = 4;           // points per batch of independent loads of the analysis (the compiler also hoists
                                // the batch's twiddle reads: a larger batch spills)
constexpr int SP = 8;           // points per thread of the synthesis
constexpr int SMP = 16;         // modes per twiddle pass of the synthesis
constexpr int FILM1_MAXK = 64;  // conditioning scalars

// (cos, sin) of theta = 2 pi k l / L from the exact integer phase.  k l < 2^24 (k <= 128, l < 65536) is exact in
// fp32, so the quotient estimate is off by at most one and two conditional steps give k l mod L exactly (an integer
// division costs more than the sincospif it feeds).
__device__ __forceinline__ float2 twiddle1(int k, int l, int L) {
    const int kl = k * l;
    int ph = kl - (int)((float)kl * (1.0f / (float)L)) * L;
    ph = ph < 0 ? ph + L : ph;
    ph = ph >= L ? ph - L : ph;
    float s, c;
    sincospif(2.0f * (float)ph / (float)L, &s, &c);
    return make_float2(c, s);
}

struct Srcs1 {
    const float* ptr[NPS_MAX_SRC];
    int C[NPS_MAX_SRC];
    int nsrc;
};

// the c2r weight of bin k: DC and (even L) Nyquist count once, every other bin twice
__device__ __forceinline__ float bin_weight(int k, int L) { return (k == 0 || 2 * k == L) ? 1.f : 2.f; }

// Analysis partials.  Thread (q, slot): q = tid % QL is the channel quad of the group, slot = tid / QL = (ls, mg):
// sub-chunk ls of the work-group's run (LS points each) and mode group mg (MK modes) of the pass.  Slot (0, mg) adds
// the sums of slots (1, mg), (2, mg), ... in that order (handed over in LDS, one of the quad's channels per round)
// and stores.  dst is [B][NP][m][C] complex with NP = gridDim.x partials per sample (NP == 1: dst is X itself and
// the adjoint's bin scale applies here).
// ALIGNED: every source has C % 4 == 0, so a quad is one 16-B load from one source.
template <int MK, bool ALIGNED>
__global__ __launch_bounds__(256, 2) void dft1d_kernel(Srcs1 S, int L, int C, int m, int QL, int LS, int nls, int nmgp,
                                                    int NP, float2* __restrict__ dst, int adj) {
    extern __shared__ __attribute__((aligned(16))) float2 tw[];  // [nls][PT][nmgp * MK]; then the hand-over buffer
    const int q = threadIdx.x % QL, slot = threadIdx.x / QL;
    const int ls = slot / nmgp, mg = slot - ls * nmgp;
    const bool live = ls < nls;
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * QL * 4 + 4 * q;
    const int MP = nmgp * MK;  // modes per pass
    const float inv_mp = 1.0f / (float)MP;
    // this thread's four channels: pointer at (b, l = 0) and the point stride of the source
    const float* cp[4] = {nullptr, nullptr, nullptr, nullptr};
    int cs[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        int lo = 0;
        for (int s = 0; s < S.nsrc; ++s) {
            if (c >= lo && c < lo + S.C[s] && c < C) {
                cs[i] = S.C[s];
                cp[i] = S.ptr[s] + (size_t)b * L * S.C[s] + (c - lo);
            }
            lo += S.C[s];
        }
    }
    const int p = blockIdx.x * nls + ls;  // this slot's sub-chunk: points [l0, lend)
    const int l0 = p * LS;
    const int lend = live ? min(L, l0 + LS) : 0;
    // XB points from lb on (zero past the sub-chunk): independent loads, issued before their FMAs (issuing them a
    // whole batch ahead measured no gain: the kernel is not bound by load latency)
    auto load_batch = [&](f32x4(&d)[XB], int lb) {
#pragma unroll
        for (int j = 0; j < XB; ++j) {
            const int l = lb + j;
            d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (l < lend) {
                if (ALIGNED) {
                    if (cp[0] != nullptr) d[j] = *reinterpret_cast<const f32x4*>(cp[0] + (size_t)l * cs[0]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (cp[i] != nullptr) d[j][i] = cp[i][(size_t)l * cs[i]];
                }
            }
        }
    };
    for (int k0 = 0; k0 < m; k0 += MP) {
        float re[4][MK], im[4][MK];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < MK; ++k) re[i][k] = im[i][k] = 0.f;
        for (int t0 = 0; t0 < LS; t0 += PT) {
            __syncthreads();
            for (int e = threadIdx.x; e < nls * PT * MP; e += 256) {
                // e / MP without an integer division: e < 2^12 and MP <= 96, so (e + 0.5) / MP is never within
                // fp32 rounding of an integer and the truncation is exact
                const int r = (int)(((float)e + 0.5f) * inv_mp), kk = e - r * MP;
                const int j = r % PT, s = r / PT;
                const int l = (blockIdx.x * nls + s) * LS + t0 + j, k = k0 + kk;
                tw[e] = (l < L && k < m) ? twiddle1(k, l, L) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            if (!live || l0 + t0 >= L) continue;
            const float2* twp = tw + (size_t)(ls * PT) * MP + mg * MK;
#pragma unroll 1
            for (int jb = 0; jb < PT; jb += XB) {
                f32x4 xv[XB];
                load_batch(xv, l0 + t0 + jb);
#pragma unroll
                for (int j = 0; j < XB; ++j) {
                    const f32x4* t4 = reinterpret_cast<const f32x4*>(twp + (size_t)(jb + j) * MP);
#pragma unroll
                    for (int k2 = 0; k2 < MK / 2; ++k2) {
                        const f32x4 t = t4[k2];  // (cos, sin) of modes 2 k2, 2 k2 + 1
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            re[i][2 * k2] = fmaf(xv[j][i], t[0], re[i][2 * k2]);
                            im[i][2 * k2] = fmaf(xv[j][i], t[1], im[i][2 * k2]);
                            re[i][2 * k2 + 1] = fmaf(xv[j][i], t[2], re[i][2 * k2 + 1]);
                            im[i][2 * k2 + 1] = fmaf(xv[j][i], t[3], im[i][2 * k2 + 1]);
                        }
                    }
                }
            }
        }
        if (nls > 1) {
            float* red = reinterpret_cast<float*>(tw);  // [2 MK][nt]: value-major, so lanes hit distinct banks
            const int nt = (nls - 1) * nmgp * QL;
            const int t = ((ls - 1) * nmgp + mg) * QL + q;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __syncthreads();  // the twiddle tile (or the previous round) has been read
                if (live && ls > 0) {
#pragma unroll
                    for (int kk = 0; kk < MK; ++kk) {
                        red[(2 * kk) * nt + t] = re[i][kk];
                        red[(2 * kk + 1) * nt + t] = im[i][kk];
                    }
                }
                __syncthreads();
                if (ls == 0) {
#pragma unroll 1
                    for (int s2 = 1; s2 < nls; ++s2) {
                        const int t2 = ((s2 - 1) * nmgp + mg) * QL + q;
#pragma unroll
                        for (int kk = 0; kk < MK; ++kk) {
                            re[i][kk] += red[(2 * kk) * nt + t2];
                            im[i][kk] += red[(2 * kk + 1) * nt + t2];
                        }
                    }
                }
            }
        }
        if (ls != 0) continue;
        float2* d = dst + ((size_t)b * NP + blockIdx.x) * m * C;
#pragma unroll
        for (int kk = 0; kk < MK; ++kk) {
            const int k = k0 + mg * MK + kk;
            if (k >= m) continue;
            const float f = (NP == 1 && adj) ? bin_weight(k, L) / (float)L : 1.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < C) d[(size_t)k * C + c0 + i] = make_float2(re[i][kk] * f, -im[i][kk] * f);
        }
    }
}

// X[b][k][c] = f_k * sum_p P[b][p][k][c], p ascending; f_k = c_k / L for the synthesis adjoint, else 1
__global__ void dft1d_reduce_kernel(const float2* __restrict__ P, float2* __restrict__ X, int L, int C, int m, int NP,
                                    int adj, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t mc = (size_t)m * C;
    const size_t b = i / mc, r = i - b * mc;
    const int k = (int)(r / C);
    const float2* src = P + b * NP * mc + r;
    float2 acc = src[0];
    for (int p = 1; p < NP; ++p) {
        const float2 v = src[(size_t)p * mc];
        acc.x += v.x;
        acc.y += v.y;
    }
    const float f = adj ? bin_weight(k, L) / (float)L : 1.f;
    X[i] = make_float2(acc.x * f, acc.y * f);
}

// out[b][l][o] (=|+=) act( scale * sum_k c_k Re(Z[b][k][o] e^{+2 pi i k l / L}) [+ addend] ); adj: c_k = 1 and
// scale = 1, the adjoint of the analysis (gX -> gx).  Thread (q, slot): channel quad q of the group, points
// slot * SP .. + SP - 1 of each tile of nslot * SP points; the work-group walks `tiles` tiles.
template <bool QUAD>
__global__ __launch_bounds__(256) void idft1d_kernel(const float2* __restrict__ Z, float* __restrict__ out, int L,
                                                     int Cout, int m, int QL, int tiles, int accumulate,
                                                     const float* __restrict__ addend, int act, int adj) {
    extern __shared__ __attribute__((aligned(16))) float lds1[];
    const int CG = QL * 4, nslot = 256 / QL, TP = nslot * SP;  // QL = 16 or 32: all powers of two
    const int cg_sh = __builtin_ctz(CG), tp_sh = __builtin_ctz(TP);
    float* zre = lds1;                                              // [m][CG]
    float* zim = lds1 + (size_t)m * CG;                             // [m][CG]
    float2* tw = reinterpret_cast<float2*>(lds1 + (size_t)2 * m * CG);  // [SMP][TP]
    const int q = threadIdx.x % QL, slot = threadIdx.x / QL;
    const int b = blockIdx.z, cbase = blockIdx.y * CG;
    for (int e = threadIdx.x; e < m * CG; e += 256) {
        const int k = e >> cg_sh, cl = e & (CG - 1);
        float2 z = make_float2(0.f, 0.f);
        if (cbase + cl < Cout) z = Z[((size_t)b * m + k) * Cout + cbase + cl];
        const bool self_conj = (k == 0) || (2 * k == L);
        const float cm = (self_conj || adj) ? 1.f : 2.f;
        zre[e] = z.x * cm;
        zim[e] = self_conj ? 0.f : z.y * cm;  // irfft drops Im of DC / Nyquist (their sines are exact zeros anyway)
    }
    const float scale = adj ? 1.f : 1.f / (float)L;
    const int c0 = cbase + 4 * q;
    for (int t = 0; t < tiles; ++t) {
        const int lt = (blockIdx.x * tiles + t) * TP;  // first point of the tile (uniform)
        if (lt >= L) break;
        f32x4 acc[SP];
#pragma unroll
        for (int j = 0; j < SP; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < m; k0 += SMP) {
            __syncthreads();
            for (int e = threadIdx.x; e < SMP * TP; e += 256) {
                const int kk = e >> tp_sh, j = e & (TP - 1);
                const int k = k0 + kk, l = lt + j;
                tw[e] = (k < m && l < L) ? twiddle1(k, l, L) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            const int nk = min(SMP, m - k0);
            for (int kk = 0; kk < nk; ++kk) {
                const f32x4 zr = *reinterpret_cast<const f32x4*>(zre + (size_t)(k0 + kk) * CG + 4 * q);
                const f32x4 zi = *reinterpret_cast<const f32x4*>(zim + (size_t)(k0 + kk) * CG + 4 * q);
                const f32x4* t4 = reinterpret_cast<const f32x4*>(tw + (size_t)kk * TP + slot * SP);
#pragma unroll
                for (int j2 = 0; j2 < SP / 2; ++j2) {
                    const f32x4 tv = t4[j2];  // (cos, sin) of points 2 j2, 2 j2 + 1
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[2 * j2][i] = fmaf(zr[i], tv[0], fmaf(-zi[i], tv[1], acc[2 * j2][i]));
                        acc[2 * j2 + 1][i] = fmaf(zr[i], tv[2], fmaf(-zi[i], tv[3], acc[2 * j2 + 1][i]));
                    }
                }
            }
        }
        if (c0 >= Cout) continue;
#pragma unroll
        for (int j = 0; j < SP; ++j) {
            const int l = lt + slot * SP + j;
            if (l >= L) continue;
            const size_t at = ((size_t)b * L + l) * Cout + c0;
            if (QUAD) {  // Cout % 4 == 0: the quad is one aligned 16-B access
                f32x4 v = acc[j] * scale;
                if (accumulate) v += *reinterpret_cast<const f32x4*>(out + at);
                if (addend != nullptr) v += *reinterpret_cast<const f32x4*>(addend + at);
                if (act == 1)
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = nps::gelu_erf(v[i]);
                *reinterpret_cast<f32x4*>(out + at) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (c0 + i >= Cout) continue;
                    float v = acc[j][i] * scale;
                    if (accumulate) v += out[at + i];
                    if (addend != nullptr) v += addend[at + i];
                    if (act == 1) v = nps::gelu_erf(v);
                    out[at + i] = v;
                }
            }
        }
    }
}

// wp[k][i][o] = w[i][o][k] (complex), and its adjoint
__global__ void pack1d_kernel(const float2* __restrict__ w, float2* __restrict__ wp, int Cin, int Cout, int m,
                              int unpack) {
    const size_t n = (size_t)Cin * Cout * m;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    // idx runs over the written tensor, so stores coalesce
    if (!unpack) {
        const int o = idx % Cout;
        const size_t t = idx / Cout;
        const int i = t % Cin, k = (int)(t / Cin);
        wp[idx] = w[((size_t)i * Cout + o) * m + k];
    } else {
        const int k = idx % m;
        const size_t t = idx / m;
        const int o = t % Cout, i = (int)(t / Cout);
        wp[idx] = w[((size_t)k * Cin + i) * Cout + o];
    }
}

// S[b][k][o] = [mode 0] 1 + bias[n] + sum_j p[b][j] wf[n][j], n = o m + k (weights_feat(p).view(B, Cout, m))
__global__ void film1d_scale_kernel(const float* __restrict__ p, const float* __restrict__ wf,
                                    const float* __restrict__ bias, float* __restrict__ S, int K, int Cout, int m,
                                    int mode, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int o = idx % Cout;
    const size_t t = idx / Cout;
    const int k = t % m;
    const size_t b = t / m;
    const size_t n = (size_t)o * m + k;
    float acc = bias[n];
    for (int j = 0; j < K; ++j) acc = fmaf(p[b * K + j], wf[n * K + j], acc);
    S[idx] = mode == 0 ? 1.0f + acc : acc;
}

// gwf[n][j] = sum_b gS[b][k][o] p[b][j], gbias[n] = sum_b gS[b][k][o] (j == K): one thread per (n, j), the batch
// walked in order with an fp64 sum
__global__ void film1d_wgrad_kernel(const float* __restrict__ gS, const float* __restrict__ p, float* __restrict__ gwf,
                                    float* __restrict__ gbias, int B, int K, int Cout, int m) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over (j, k, o), o fastest
    const size_t per = (size_t)m * Cout;
    if (idx >= per * (K + 1)) return;
    const int j = (int)(idx / per);
    const size_t r = idx - (size_t)j * per;
    const int k = (int)(r / Cout), o = (int)(r - (size_t)k * Cout);
    const size_t n = (size_t)o * m + k;
    float* dst = j < K ? (gwf ? gwf + n * K + j : nullptr) : (gbias ? gbias + n : nullptr);
    if (dst == nullptr) return;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += (double)gS[(size_t)b * per + r] * (j < K ? (double)p[(size_t)b * K + j] : 1.0);
    *dst = (float)acc;
}

// gp[b][j] = sum_n gS[b][k][o] wf[n][j]: work-group (j, b); fp64 per-thread sums, one fixed-order block sum
__global__ __launch_bounds__(256) void film1d_pgrad_kernel(const float* __restrict__ gS, const float* __restrict__ wf,
                                                           float* __restrict__ gp, int K, int Cout, int m) {
    __shared__ double scratch[4];
    const int j = blockIdx.x, b = blockIdx.y;
    const int N = Cout * m;
    double acc = 0.0;
    for (int e = threadIdx.x; e < N; e += 256) {  // e over (k, o), o fastest: coalesced gS
        const int k = e / Cout, o = e - k * Cout;
        acc += (double)gS[(size_t)b * N + e] * (double)wf[((size_t)o * m + k) * K + j];
    }
    const double tot = nps::block_sum(acc, scratch);
    if (threadIdx.x == 0) gp[(size_t)b * K + j] = (float)tot;
}

// ---- host side -----------------------------------------------------------------------------------------------

bool shape_ok(const char* what, int B, int L, int m) {
    if (!(B > 0 && B <= 65535)) {
        nps::set_error("%s: B must be in [1, 65535], got %d", what, B);
    } else if (!(L >= 2 && L <= MAX_L)) {
        nps::set_error("%s: L must be in [2, %d], got %d", what, MAX_L, L);
    } else if (!(m >= 1 && m <= MAX_M)) {
        nps::set_error("%s: modes must be in [1, %d], got %d", what, MAX_M, m);
    } else if (!(m <= L / 2 + 1)) {
        nps::set_error("%s: modes should be at most the spatial dim // 2 + 1 (L=%d m=%d)", what, L, m);
    } else {
        return true;
    }
    return false;
}

bool film1_ok(const char* what, int K, int mode) {
    if (!(K > 0 && K <= FILM1_MAXK)) {
        nps::set_error("%s: K (feature_transform_dim) must be in [1, %d], got %d", what, FILM1_MAXK, K);
    } else if (!(mode == 0 || mode == 1)) {
        nps::set_error("%s: transform_mode is 0 (1 + FiLM) or 1 (FiLM), got %d", what, mode);
    } else {
        return true;
    }
    return false;
}

// The analysis plan: quad lanes QL (channels per group = 4 QL), modes per thread MK, mode groups per pass nmgp,
// sub-chunks per work-group nls, points per sub-chunk LS, partials (= work-groups) per sample NP.
struct Plan1 {
    int QL, MK, nmgp, nls, LS, NP, gx, gy;
};
Plan1 plan_dft(int B, int L, int C, int m) {
    Plan1 p;
    p.QL = C <= 64 ? 16 : 32;
    const int nslot = 256 / p.QL;
    double best = -1.0;
    const int mks[2] = {8, 12};  // (16 modes x 4 channels x re / im does not fit the register file)
    for (int i = 0; i < 2; ++i) {  // the mode tile that leaves the fewest idle slots / padded modes
        const int MK = mks[i], nmg = (m + MK - 1) / MK;
        const int passes = (nmg + nslot - 1) / nslot, nmgp = (nmg + passes - 1) / passes;
        const int nls = nslot / nmgp;
        const double eff = (double)m / (MK * nmgp * passes) * (double)(nmgp * nls) / nslot;
        if (eff > best + 1e-9) {
            best = eff;
            p.MK = MK;
            p.nmgp = nmgp;
            p.nls = nls;
        }
    }
    p.gy = (C + 4 * p.QL - 1) / (4 * p.QL);
    p.LS = 256;  // shorter sub-chunks until the grid covers the device (more partials: a longer second pass)
    while (p.LS > 32 && (long)B * p.gy * ((L + p.nls * p.LS - 1) / (p.nls * p.LS)) < 512) p.LS /= 2;
    p.gx = (L + p.nls * p.LS - 1) / (p.nls * p.LS);
    p.NP = p.gx;  // one partial per work-group
    return p;
}

template <int MK>
void launch_dft1d(bool aligned, dim3 grid, size_t lds, hipStream_t s, const Srcs1& S, int L, int C, int m,
                  const Plan1& p, float2* dst, int adj) {
    if (aligned)
        dft1d_kernel<MK, true><<<grid, 256, lds, s>>>(S, L, C, m, p.QL, p.LS, p.nls, p.nmgp, p.NP, dst, adj);
    else
        dft1d_kernel<MK, false><<<grid, 256, lds, s>>>(S, L, C, m, p.QL, p.LS, p.nls, p.nmgp, p.NP, dst, adj);
}

size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

extern "C" size_t nps_spectral1d_dft_workspace(int B, int L, int C, int m) {
    if (!(B > 0 && B <= 65535 && C > 0 && L >= 2 && L <= MAX_L && m >= 1 && m <= MAX_M && m <= L / 2 + 1)) return 0;
    const Plan1 p = plan_dft(B, L, C, m);
    return al256((size_t)B * p.NP * m * C * sizeof(float2));
}

extern "C" int nps_spectral1d_dft(const nps_src_t* src, int nsrc, int B, int L, int C, int m, float* X, float* ws,
                                  int adjoint, void* stream) {
    NPS_CHECK_ARG(src && X && ws, "spectral1d_dft: NULL pointer");
    NPS_CHECK_ARG(nsrc >= 1 && nsrc <= NPS_MAX_SRC, "spectral1d_dft: 1 .. %d sources, got %d", NPS_MAX_SRC, nsrc);
    if (!shape_ok("spectral1d_dft", B, L, m)) return -1;
    Srcs1 S = {};
    S.nsrc = nsrc;
    int cs = 0;
    bool aligned = true;
    for (int i = 0; i < nsrc; ++i) {
        NPS_CHECK_ARG(src[i].ptr && src[i].C > 0 && src[i].H == 1 && src[i].W == L && src[i].off_y == 0 &&
                          src[i].off_x == 0,
                      "spectral1d_dft: source %d must be a (B, 1, L, C) tensor covering the frame", i);
        S.ptr[i] = src[i].ptr;
        S.C[i] = src[i].C;
        cs += src[i].C;
        aligned = aligned && (src[i].C & 3) == 0 && (reinterpret_cast<uintptr_t>(src[i].ptr) & 15) == 0;
    }
    NPS_CHECK_ARG(cs == C && C > 0, "spectral1d_dft: the sources' channels sum to %d, C is %d", cs, C);
    const Plan1 p = plan_dft(B, L, C, m);
    NPS_CHECK_ARG(p.gy <= 65535, "spectral1d_dft: C=%d too large", C);
    hipStream_t s = (hipStream_t)stream;
    float2* dst = reinterpret_cast<float2*>(p.NP == 1 ? X : ws);
    const dim3 grid(p.gx, p.gy, B);
    // the twiddle tile (<= 16 slots x 16 points x 12 modes: 24 KiB) or the sub-chunk hand-over (<= 240 threads x
    // 24 floats: 22.5 KiB), whichever is larger
    const size_t lds_tw = sizeof(float2) * p.nls * PT * p.nmgp * p.MK;
    const size_t lds_red = sizeof(float) * (p.nls - 1) * p.nmgp * p.QL * 2 * p.MK;
    const size_t lds = lds_tw > lds_red ? lds_tw : lds_red;
    switch (p.MK) {
        case 8: launch_dft1d<8>(aligned, grid, lds, s, S, L, C, m, p, dst, adjoint ? 1 : 0); break;
        default: launch_dft1d<12>(aligned, grid, lds, s, S, L, C, m, p, dst, adjoint ? 1 : 0); break;
    }
    NPS_CHECK_LAUNCH("spectral1d_dft");
    if (p.NP > 1) {
        const size_t n = (size_t)B * m * C;
        dft1d_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(reinterpret_cast<const float2*>(ws),
                                                                       reinterpret_cast<float2*>(X), L, C, m, p.NP,
                                                                       adjoint ? 1 : 0, n);
        NPS_CHECK_LAUNCH("spectral1d_dft (reduce)");
    }
    return 0;
}

extern "C" int nps_spectral1d_idft(const float* Z, float* out, int B, int L, int m, int Cout, int accumulate,
                                   const float* addend, int act, int adjoint, void* stream) {
    NPS_CHECK_ARG(Z && out, "spectral1d_idft: NULL pointer");
    if (!shape_ok("spectral1d_idft", B, L, m)) return -1;
    NPS_CHECK_ARG(Cout > 0, "spectral1d_idft: Cout must be positive, got %d", Cout);
    NPS_CHECK_ARG(act == 0 || act == 1, "spectral1d_idft: act is 0 (none) or 1 (GELU)");
    // channels per group: the group's Z [m][CG] complex stays within 64 KiB of LDS
    const int QL = (Cout > 64 && m <= 64) ? 32 : 16;
    const int CG = 4 * QL, TP = (256 / QL) * SP;
    const int gy = (Cout + CG - 1) / CG;
    NPS_CHECK_ARG(gy <= 65535, "spectral1d_idft: Cout=%d too large", Cout);
    int tiles = 8;  // more tiles per work-group amortise the Z staging; fewer keep the device covered
    while (tiles > 1 && (long)B * gy * ((L + tiles * TP - 1) / (tiles * TP)) < 512) tiles /= 2;
    const dim3 grid((L + tiles * TP - 1) / (tiles * TP), gy, B);
    const size_t lds = sizeof(float) * 2 * m * CG + sizeof(float2) * SMP * TP;  // <= 64 KiB + 16 KiB
    static bool attr_set = false;
    if (!attr_set) {  // more than the 64 KiB a kernel gets by default
        (void)hipFuncSetAttribute((const void*)idft1d_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  96 * 1024);
        (void)hipFuncSetAttribute((const void*)idft1d_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  96 * 1024);
        attr_set = true;
    }
    hipStream_t s = (hipStream_t)stream;
    const auto* z = reinterpret_cast<const float2*>(Z);
    const bool quad = (Cout & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(addend) & 15) == 0;
    if (quad)
        idft1d_kernel<true><<<grid, 256, lds, s>>>(z, out, L, Cout, m, QL, tiles, accumulate ? 1 : 0, addend, act,
                                                   adjoint ? 1 : 0);
    else
        idft1d_kernel<false><<<grid, 256, lds, s>>>(z, out, L, Cout, m, QL, tiles, accumulate ? 1 : 0, addend, act,
                                                    adjoint ? 1 : 0);
    NPS_CHECK_LAUNCH("spectral1d_idft");
    return 0;
}

extern "C" int nps_spectral1d_pack_weights(const float* w, float* wpack, int Cin, int Cout, int m, void* stream) {
    NPS_CHECK_ARG(w && wpack && Cin > 0 && Cout > 0 && m > 0, "spectral1d_pack_weights: bad args");
    const size_t n = (size_t)Cin * Cout * m;
    pack1d_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float2*>(w), reinterpret_cast<float2*>(wpack), Cin, Cout, m, 0);
    NPS_CHECK_LAUNCH("spectral1d_pack_weights");
    return 0;
}

extern "C" int nps_spectral1d_unpack_grad(const float* gwpack, float* gw, int Cin, int Cout, int m, void* stream) {
    NPS_CHECK_ARG(gwpack && gw && Cin > 0 && Cout > 0 && m > 0, "spectral1d_unpack_grad: bad args");
    const size_t n = (size_t)Cin * Cout * m;
    pack1d_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float2*>(gwpack), reinterpret_cast<float2*>(gw), Cin, Cout, m, 1);
    NPS_CHECK_LAUNCH("spectral1d_unpack_grad");
    return 0;
}

// The mixer's backward at any batch size: nps_spectral_mix_bwd on runs of 32 samples (its MFMA kernel's reach; the
// scalar kernel's LDS holds B x Cout), each run's weight gradient into its own part, then the parts added into
// part 0 in ascending order.
namespace {
constexpr int MIXB_RUN = 32;
__global__ void sum_parts_kernel(float* __restrict__ g, int parts, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = g[i];
    for (int p = 1; p < parts; ++p) acc += g[(size_t)p * n + i];
    g[i] = acc;
}
}  // namespace

extern "C" int nps_spectral1d_mix_bwd_parts(int B) { return B > 0 ? (B + MIXB_RUN - 1) / MIXB_RUN : 0; }

extern "C" int nps_spectral1d_mix_bwd(const float* X, const float* wpack, const float* gY, float* gX, float* gwpack,
                                      int B, int m, int Cin, int Cout, void* stream) {
    NPS_CHECK_ARG(X && wpack && gY && gX && gwpack, "spectral1d_mix_bwd: NULL pointer");
    NPS_CHECK_ARG(B > 0 && m > 0 && Cin > 0 && Cout > 0,
                  "spectral1d_mix_bwd: sizes must be positive (B=%d m=%d Cin=%d Cout=%d)", B, m, Cin, Cout);
    const size_t nw = (size_t)m * Cin * Cout * 2;  // floats per part
    const int parts = nps_spectral1d_mix_bwd_parts(B);
    for (int c = 0; c < parts; ++c) {
        const int b0 = c * MIXB_RUN, nb = B - b0 < MIXB_RUN ? B - b0 : MIXB_RUN;
        const int rc = nps_spectral_mix_bwd(X + (size_t)b0 * m * Cin * 2, wpack, gY + (size_t)b0 * m * Cout * 2,
                                            gX + (size_t)b0 * m * Cin * 2, gwpack + c * nw, nb, 1, m, Cin, Cout,
                                            stream);
        if (rc < 0) return rc;
    }
    if (parts > 1) {
        sum_parts_kernel<<<(unsigned)((nw + 255) / 256), 256, 0, (hipStream_t)stream>>>(gwpack, parts, nw);
        NPS_CHECK_LAUNCH("spectral1d_mix_bwd (parts)");
    }
    return 0;
}

extern "C" int nps_spectral1d_film_scale(const float* p, const float* wf, const float* bias, float* S, int B, int K,
                                         int Cout, int m, int transform_mode, void* stream) {
    NPS_CHECK_ARG(p && wf && bias && S, "spectral1d_film_scale: NULL pointer");
    NPS_CHECK_ARG(B > 0 && Cout > 0 && m > 0 && (size_t)Cout * m <= (size_t)INT_MAX,
                  "spectral1d_film_scale: B, Cout and m must be positive and Cout*m fit an int (B=%d Cout=%d m=%d)", B,
                  Cout, m);
    if (!film1_ok("spectral1d_film_scale", K, transform_mode)) return -1;
    const size_t n = (size_t)B * m * Cout;
    film1d_scale_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(p, wf, bias, S, K, Cout, m,
                                                                                     transform_mode, n);
    NPS_CHECK_LAUNCH("spectral1d_film_scale");
    return 0;
}

extern "C" int nps_spectral1d_film_param_bwd(const float* gS, const float* p, const float* wf, float* gwf,
                                             float* gbias, float* gp, int B, int K, int Cout, int m,
                                             int transform_mode, void* stream) {
    NPS_CHECK_ARG(gS && p && wf, "spectral1d_film_param_bwd: NULL pointer");
    NPS_CHECK_ARG(B > 0 && B <= 65535 && Cout > 0 && m > 0 && (size_t)Cout * m <= (size_t)INT_MAX,
                  "spectral1d_film_param_bwd: B in [1, 65535], Cout and m positive, Cout*m fitting an int (B=%d "
                  "Cout=%d m=%d)", B, Cout, m);
    if (!film1_ok("spectral1d_film_param_bwd", K, transform_mode)) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (gwf != nullptr || gbias != nullptr) {
        const size_t n = (size_t)m * Cout * (K + 1);
        film1d_wgrad_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(gS, p, gwf, gbias, B, K, Cout, m);
        NPS_CHECK_LAUNCH("spectral1d_film_param_bwd (weights_feat)");
    }
    if (gp != nullptr) {
        film1d_pgrad_kernel<<<dim3(K, B), 256, 0, s>>>(gS, wf, gp, K, Cout, m);
        NPS_CHECK_LAUNCH("spectral1d_film_param_bwd (p)");
    }
    return 0;
}

// ---- one call per module -------------------------------------------------------------------------------------
namespace {

struct Film1 {
    const float *p, *wf, *bias;
    int K, mode;
};

struct Sz1 {
    size_t wp, part, x, y, gwp;  // wpack [m][Cin][Cout], the analysis partials (of the wider of Cin / Cout),
                                 // X [B][m][Cin], Y [B][m][Cout], the weight-gradient parts of the mixer's backward
};
Sz1 sizes1(int B, int Cin, int Cout, int L, int m) {
    Sz1 s;
    s.wp = (size_t)m * Cin * Cout * 8;
    const size_t pa = nps_spectral1d_dft_workspace(B, L, Cin, m), pb = nps_spectral1d_dft_workspace(B, L, Cout, m);
    s.part = pa > pb ? pa : pb;
    s.x = (size_t)B * m * Cin * 8;
    s.y = (size_t)B * m * Cout * 8;
    s.gwp = s.wp * (size_t)nps_spectral1d_mix_bwd_parts(B);
    return s;
}
// [wp][partials][X][Y][gX][gwp], FiLM adds [S][Yu][gS]
size_t ws1(const Sz1& s) { return al256(s.wp) + al256(s.part) + al256(s.x) + al256(s.y) + al256(s.x) + al256(s.gwp); }
size_t film_ws1(const Sz1& s) { return ws1(s) + al256(s.y / 2) + al256(s.y) + al256(s.y / 2); }

struct Carve1 {
    char* base;
    size_t off = 0;
    float* take(size_t bytes) {
        float* p = reinterpret_cast<float*>(base + off);
        off += al256(bytes);
        return p;
    }
};

bool args1_ok(const char* what, int B, int Cin, int Cout, int L, int m) {
    if (!(Cin > 0 && Cout > 0)) {
        nps::set_error("%s: Cin and Cout must be positive (Cin=%d Cout=%d)", what, Cin, Cout);
        return false;
    }
    return shape_ok(what, B, L, m);
}

int conv1d_fwd(const char* what, const float* x, const float* w, float* y, void* ws, int B, int Cin, int Cout, int L,
               int m, int accumulate, int act, void* stream, const Film1* film) {
    NPS_CHECK_ARG(x && w && y && ws, "%s: NULL pointer", what);
    if (film != nullptr) {
        NPS_CHECK_ARG(film->p && film->wf && film->bias, "%s: NULL FiLM pointer (p, wf, bias)", what);
        if (!film1_ok(what, film->K, film->mode)) return -1;
    }
    if (!args1_ok(what, B, Cin, Cout, L, m)) return -1;
    NPS_CHECK_ARG(act == 0 || act == 1, "%s: act is 0 (none) or 1 (GELU)", what);
    const Sz1 sz = sizes1(B, Cin, Cout, L, m);
    Carve1 c{static_cast<char*>(ws)};
    float* wp = c.take(sz.wp);
    float* part = c.take(sz.part);
    float* X = c.take(sz.x);
    float* Y = c.take(sz.y);
    float* S = film ? reinterpret_cast<float*>(static_cast<char*>(ws) + ws1(sz)) : nullptr;
    const nps_src_t src = {x, Cin, 1, L, 0, 0};
    int rc;
    if ((rc = nps_spectral1d_pack_weights(w, wp, Cin, Cout, m, stream)) < 0) return rc;
    if ((rc = nps_spectral1d_dft(&src, 1, B, L, Cin, m, X, part, 0, stream)) < 0) return rc;
    if (film != nullptr) {
        if ((rc = nps_spectral1d_film_scale(film->p, film->wf, film->bias, S, B, film->K, Cout, m, film->mode,
                                            stream)) < 0)
            return rc;
        if ((rc = nps_spectral_mix_scaled(X, wp, S, Y, B, 1, m, Cin, Cout, stream)) < 0) return rc;
    } else if ((rc = nps_spectral_mix(X, wp, Y, B, 1, m, Cin, Cout, stream)) < 0) {
        return rc;
    }
    return nps_spectral1d_idft(Y, y, B, L, m, Cout, accumulate ? 1 : 0, nullptr, act, 0, stream);
}

int conv1d_bwd(const char* what, const float* x, const float* w, const float* dy, float* dx, float* dw, void* ws,
               int B, int Cin, int Cout, int L, int m, void* stream, const Film1* film, float* dp, float* dwf,
               float* dbias) {
    NPS_CHECK_ARG(x && w && dy && ws, "%s: NULL pointer", what);
    if (film != nullptr) {
        NPS_CHECK_ARG(film->p && film->wf && film->bias, "%s: NULL FiLM pointer (p, wf, bias)", what);
        if (!film1_ok(what, film->K, film->mode)) return -1;
    }
    if (!args1_ok(what, B, Cin, Cout, L, m)) return -1;
    const Sz1 sz = sizes1(B, Cin, Cout, L, m);
    Carve1 c{static_cast<char*>(ws)};
    float* wp = c.take(sz.wp);
    float* part = c.take(sz.part);
    float* X = c.take(sz.x);
    float* gY = c.take(sz.y);
    float* gX = c.take(sz.x);
    float* gwp = c.take(sz.gwp);
    float* S = film ? c.take(sz.y / 2) : nullptr;
    float* Yu = film ? c.take(sz.y) : nullptr;
    float* gS = film ? c.take(sz.y / 2) : nullptr;
    const nps_src_t src = {x, Cin, 1, L, 0, 0}, gsrc = {dy, Cout, 1, L, 0, 0};
    int rc;
    if ((rc = nps_spectral1d_pack_weights(w, wp, Cin, Cout, m, stream)) < 0) return rc;
    if ((rc = nps_spectral1d_dft(&src, 1, B, L, Cin, m, X, part, 0, stream)) < 0) return rc;
    if ((rc = nps_spectral1d_dft(&gsrc, 1, B, L, Cout, m, gY, part, 1, stream)) < 0) return rc;  // irfft's adjoint
    if (film != nullptr) {
        // the factor and the unscaled mixer output again (never Y / S: S may be zero); gS from them, gY <- gY * S
        if ((rc = nps_spectral1d_film_scale(film->p, film->wf, film->bias, S, B, film->K, Cout, m, film->mode,
                                            stream)) < 0)
            return rc;
        if ((rc = nps_spectral_mix(X, wp, Yu, B, 1, m, Cin, Cout, stream)) < 0) return rc;
        if ((rc = nps_spectral_film_bwd(Yu, S, gY, gS, B, 1, m, Cout, stream)) < 0) return rc;
        if (dp != nullptr || dwf != nullptr || dbias != nullptr)
            if ((rc = nps_spectral1d_film_param_bwd(gS, film->p, film->wf, dwf, dbias, dp, B, film->K, Cout, m,
                                                    film->mode, stream)) < 0)
                return rc;
    }
    if ((rc = nps_spectral1d_mix_bwd(X, wp, gY, gX, gwp, B, m, Cin, Cout, stream)) < 0) return rc;
    if (dx != nullptr)
        if ((rc = nps_spectral1d_idft(gX, dx, B, L, m, Cin, 0, nullptr, 0, 1, stream)) < 0) return rc;
    if (dw != nullptr)
        if ((rc = nps_spectral1d_unpack_grad(gwp, dw, Cin, Cout, m, stream)) < 0) return rc;
    return 0;
}

}  // namespace

extern "C" size_t nps_spectral_conv1d_workspace(int B, int Cin, int Cout, int L, int m) {
    if (!(Cin > 0 && Cout > 0) || nps_spectral1d_dft_workspace(B, L, Cin, m) == 0) return 0;
    return ws1(sizes1(B, Cin, Cout, L, m));
}

extern "C" size_t nps_spectral_conv1d_film_workspace(int B, int Cin, int Cout, int L, int m) {
    if (!(Cin > 0 && Cout > 0) || nps_spectral1d_dft_workspace(B, L, Cin, m) == 0) return 0;
    return film_ws1(sizes1(B, Cin, Cout, L, m));
}

extern "C" int nps_spectral_conv1d_fwd(const float* x, const float* w, float* y, void* ws, int B, int Cin, int Cout,
                                       int L, int m, int accumulate, int act, void* stream) {
    return conv1d_fwd("spectral_conv1d_fwd", x, w, y, ws, B, Cin, Cout, L, m, accumulate, act, stream, nullptr);
}

extern "C" int nps_spectral_conv1d_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, void* ws,
                                       int B, int Cin, int Cout, int L, int m, void* stream) {
    return conv1d_bwd("spectral_conv1d_bwd", x, w, dy, dx, dw, ws, B, Cin, Cout, L, m, stream, nullptr, nullptr,
                      nullptr, nullptr);
}

extern "C" int nps_spectral_conv1d_film_fwd(const float* x, const float* w, const float* p, const float* wf,
                                            const float* bias, float* y, void* ws, int B, int Cin, int Cout, int L,
                                            int m, int K, int transform_mode, int accumulate, int act, void* stream) {
    const Film1 f = {p, wf, bias, K, transform_mode};
    return conv1d_fwd("spectral_conv1d_film_fwd", x, w, y, ws, B, Cin, Cout, L, m, accumulate, act, stream, &f);
}

extern "C" int nps_spectral_conv1d_film_bwd(const float* x, const float* w, const float* p, const float* wf,
                                            const float* bias, const float* dy, float* dx, float* dw, float* dp,
                                            float* dwf, float* dbias, void* ws, int B, int Cin, int Cout, int L, int m,
                                            int K, int transform_mode, void* stream) {
    const Film1 f = {p, wf, bias, K, transform_mode};
    return conv1d_bwd("spectral_conv1d_film_bwd", x, w, dy, dx, dw, ws, B, Cin, Cout, L, m, stream, &f, dp, dwf,
                      dbias);
}
