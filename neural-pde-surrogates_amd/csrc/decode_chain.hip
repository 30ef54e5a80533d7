// The grid decoders' per-pixel chain for gfx950 (include/nps.h, nps_decode_t): up to two Conv1d stages over a
// pixel's signal x[ci][l] (a strided Conv1d, an optional GELU / Swish, a stride-1 Conv1d), then add_delta in its
// three modes, the wrapper's tanh and the obstacle mask -- forward and backward.  TimeConvLinear is one stage, TimeConv
// and TimeConvDense ('all' / 'none') are two, LinearConv's epilogue and add_delta itself are none.
//
// Layout.  A work-group of 256 threads owns PX consecutive pixels of one sample (PX = 64, 32, 16 or 8: the largest
// whose tiles fit the 160 KiB of LDS); thread = (pixel p = tid % PX, slot = tid / PX).  Every per-pixel array lives in
// LDS as [p][pitch] with an odd pitch, so a lane walking its own row never meets another lane's bank:
//   xs  [PX][C0*L0 | 1]  the input tile.  Planar input (x_ps == 1) is loaded with consecutive lanes on consecutive
//                        pixels, channels-last input with consecutive lanes on consecutive (ci, l): both are coalesced
//                        runs in memory, and both LDS write patterns are conflict-free with the odd pitch.
//   a1s [PX][C1*L1 | 1]  act(stage 1) when a second stage follows (8 x 34 floats per pixel for TimeConv at tw = 25:
//                        too many for VGPRs next to the accumulators).
// The slots share out the (channel, position) outputs of each stage; with PX = 64 a slot is a wave, its output index is
// wave-uniform and the weights arrive through scalar loads.  Sizes are runtime values throughout.
//
// Backward.  A work-group walks pixel groups grid-stride; per group it recomputes the chain, keeps act and act' in LDS
// (a1s, gzs), forms the gradient of the chain's output (g2s), and back-propagates.  Weight and bias gradients: each
// (parameter, group) term is summed over the group's pixels with an fp64 wave reduction (as nps_timeconv_decode_bwd
// does), accumulated over the work-group's groups in an LDS accumulator owned by one thread per parameter, written as
// this work-group's row of ws, and the rows are summed in a fixed order by decode_reduce_kernel.  No atomics: two runs
// give identical bits.
#include "nps_common.hpp"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr size_t kLdsBudget = 160 * 1024;
constexpr int kBwdBlocks = 1024;  // rows of ws at most (4 work-groups' worth of groups per CU of a 256-CU device)

__device__ __forceinline__ float act_fwd(int act, float beta, float z) {
    if (act == NPS_DECODE_ACT_GELU) return nps::gelu_erf(z);
    if (act == NPS_DECODE_ACT_SWISH) return z / (1.0f + expf(-beta * z));
    return z;
}

// act(z) and its derivative
__device__ __forceinline__ void act_both(int act, float beta, float z, float& a, float& da) {
    if (act == NPS_DECODE_ACT_GELU) {
        a = nps::gelu_erf(z);
        da = nps::gelu_erf_grad(z);
    } else if (act == NPS_DECODE_ACT_SWISH) {
        const float s = 1.0f / (1.0f + expf(-beta * z));
        a = z * s;
        da = s + beta * z * s * (1.0f - s);
    } else {
        a = z;
        da = 1.0f;
    }
}

// add_delta (dec_grid.py:8-31) + tanh + mask (activation_wrapper.py:34-35) of one chain output
__device__ __forceinline__ float epilogue(const nps_decode_t& d, float delta, float ulast, int t, float m) {
    float v = delta;
    if (d.delta_mode == NPS_DECODE_PER_STEP)
        v = ulast + d.dtcum[t] * delta;
    else if (d.delta_mode == NPS_DECODE_ALL)
        v = ulast + d.dt * delta;
    if (d.act_tanh) v = tanhf(v);
    if (d.mask) v = v - m * v;
    return v;
}

// gradient of the chain output `delta` given g = dL/d(out)
__device__ __forceinline__ float epilogue_grad(const nps_decode_t& d, float delta, float ulast, int t, float m,
                                               float g) {
    float sc = 1.0f, v = delta;
    if (d.delta_mode == NPS_DECODE_PER_STEP) {
        sc = d.dtcum[t];
        v = ulast + sc * delta;
    } else if (d.delta_mode == NPS_DECODE_ALL) {
        sc = d.dt;
        v = ulast + sc * delta;
    }
    if (d.mask) g = g - m * g;
    if (d.act_tanh) {
        const float y = tanhf(v);
        g *= 1.0f - y * y;
    }
    return g * sc;
}

template <int PX>
__device__ __forceinline__ int slot_of_thread() {
    int s = threadIdx.x / PX;
    if (PX == 64) s = __builtin_amdgcn_readfirstlane(s);  // a slot is a wave: its indices are wave-uniform
    return s;
}

// Input tile of pixels [p0, p0 + np) of sample b into xs[p][XP]; rows of pixels past N are zero.
template <int PX>
__device__ __forceinline__ void load_tile(const nps_decode_t& d, int b, int p0, int np, int CL, int XP,
                                          float* __restrict__ xs) {
    const float* xb = d.x + (long)b * d.x_bs + (long)p0 * d.x_ps;
    if (d.x_ps == 1) {  // planar: lanes along pixels
        for (int i = threadIdx.x; i < CL * PX; i += kThreads) {
            const int idx = i / PX, p = i % PX;
            xs[p * XP + idx] = p < np ? xb[(long)idx * d.x_cs + p] : 0.f;
        }
    } else {  // channels-last: lanes along (ci, l)
        for (int i = threadIdx.x; i < CL * PX; i += kThreads) {
            const int p = i / CL, idx = i % CL;
            xs[p * XP + idx] = p < np ? xb[(long)p * d.x_ps + (long)idx * d.x_cs] : 0.f;
        }
    }
}

template <int PX>
__device__ __forceinline__ void store_tile(const nps_decode_t& d, float* __restrict__ gx, int b, int p0, int np,
                                           int CL, int XP, const float* __restrict__ xs) {
    float* gb = gx + (long)b * d.x_bs + (long)p0 * d.x_ps;
    if (d.x_ps == 1) {
        for (int i = threadIdx.x; i < CL * PX; i += kThreads) {
            const int idx = i / PX, p = i % PX;
            if (p < np) gb[(long)idx * d.x_cs + p] = xs[p * XP + idx];
        }
    } else {
        for (int i = threadIdx.x; i < CL * PX; i += kThreads) {
            const int p = i / CL, idx = i % CL;
            if (p < np) gb[(long)p * d.x_ps + (long)idx * d.x_cs] = xs[p * XP + idx];
        }
    }
}

// stage 1 pre-activation of output (o, t1) at this thread's pixel
__device__ __forceinline__ float stage1(const nps_decode_t& d, const float* __restrict__ xrow, int o, int t1) {
    float acc = d.b1[o];
    for (int ci = 0; ci < d.C0; ++ci) {
        const float* wr = d.w1 + (size_t)(o * d.C0 + ci) * d.k1;
        const float* xr = xrow + ci * d.L0 + t1 * d.s1;
        for (int k = 0; k < d.k1; ++k) acc = fmaf(wr[k], xr[k], acc);
    }
    return acc;
}

// stage 2 output (o2, t) at this thread's pixel
__device__ __forceinline__ float stage2(const nps_decode_t& d, const float* __restrict__ arow, int L1, int o2, int t) {
    float acc = d.b2[o2];
    for (int o = 0; o < d.C1; ++o) {
        const float* wr = d.w2 + (size_t)(o2 * d.C1 + o) * d.k2;
        const float* ar = arow + o * L1 + t;
        for (int k = 0; k < d.k2; ++k) acc = fmaf(wr[k], ar[k], acc);
    }
    return acc;
}

template <int PX>
__global__ __launch_bounds__(kThreads) void decode_fwd_kernel(const nps_decode_t d, int L1, int XP, int AP) {
    extern __shared__ float lds[];
    constexpr int NSLOT = kThreads / PX;
    const int CL = d.C0 * d.L0, NT = d.num_c * d.tw;
    float* xs = lds;                                       // [PX][XP]
    float* a1s = xs + PX * XP;                             // [PX][AP]      (two stages)
    float* uls = a1s + (d.nstage == 2 ? PX * AP : 0);      // [num_c][PX]   u at the last time step
    const int b = blockIdx.y, p0 = blockIdx.x * PX;
    const int np = min(PX, d.N - p0);
    const int p = threadIdx.x % PX, slot = slot_of_thread<PX>();
    const int pix = p0 + p;
    const bool valid = p < np;
    load_tile<PX>(d, b, p0, np, CL, XP, xs);
    if (d.delta_mode != NPS_DECODE_NONE)
        for (int c = slot; c < d.num_c; c += NSLOT)
            uls[c * PX + p] = valid ? d.u[(((size_t)b * d.num_c + c) * d.tw + (d.tw - 1)) * d.N + pix] : 0.f;
    const float m = (d.mask && valid) ? d.mask[((size_t)b * d.mask_S + d.mask_ch) * d.N + pix] : 0.f;
    __syncthreads();
    const float* xrow = xs + p * XP;
    float* arow = a1s + p * AP;
    if (d.nstage == 2) {
        for (int it = slot; it < d.C1 * L1; it += NSLOT) arow[it] = act_fwd(d.act, d.beta, stage1(d, xrow, it / L1, it % L1));
        __syncthreads();
    }
    float* ob = d.out + (size_t)b * NT * d.N + pix;
    for (int it = slot; it < NT; it += NSLOT) {
        const int c = it / d.tw, t = it % d.tw;
        float delta;
        if (d.nstage == 0)
            delta = xrow[it];
        else if (d.nstage == 1)
            delta = act_fwd(d.act, d.beta, stage1(d, xrow, c, t));
        else
            delta = stage2(d, arow, L1, c, t);
        const float ulast = d.delta_mode != NPS_DECODE_NONE ? uls[c * PX + p] : 0.f;
        const float v = epilogue(d, delta, ulast, t, m);
        if (valid) ob[(size_t)it * d.N] = v;
    }
}

// sum over the PX lanes that share a slot (fp64, like nps::wave_sum)
template <int PX>
__device__ __forceinline__ float pixel_sum(float v) {
    double s = (double)v;
#pragma unroll
    for (int o = PX / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return (float)s;
}

template <int PX>
__global__ __launch_bounds__(kThreads) void decode_bwd_kernel(const nps_decode_t d, const float* __restrict__ gout,
                                                              float* __restrict__ gx, float* __restrict__ ws,
                                                              int L1, int XP, int AP, int GP, int nparams,
                                                              int groups_per_sample, int ngroups) {
    extern __shared__ float lds[];
    constexpr int NSLOT = kThreads / PX;
    const int CL = d.C0 * d.L0, NT = d.num_c * d.tw, A = d.nstage >= 1 ? d.C1 * L1 : 0;
    float* xs = lds;                                        // [PX][XP]  input tile, then its gradient
    float* a1s = xs + PX * XP;                              // [PX][AP]  act(stage 1)
    float* gzs = a1s + (d.nstage >= 1 ? PX * AP : 0);       // [PX][AP]  act'(stage 1), then the gradient of stage 1
    float* g2s = gzs + (d.nstage >= 1 ? PX * AP : 0);       // [PX][GP]  gradient of stage 2's output
    float* uls = g2s + (d.nstage == 2 ? PX * GP : 0);       // [num_c][PX]
    float* pacc = uls + d.num_c * PX;                       // [nparams]  this work-group's parameter partials
    const int p = threadIdx.x % PX, slot = slot_of_thread<PX>();
    const bool wants_p = ws != nullptr && d.nstage >= 1;
    // parameter offsets in a row of ws: [w1 | b1 | w2 | b2] (b2 follows w2: the stage-2 loop runs over both)
    const int nw1 = d.nstage >= 1 ? d.C1 * d.C0 * d.k1 : 0, ob1 = nw1, ow2 = ob1 + (d.nstage >= 1 ? d.C1 : 0);
    const int nw2 = d.nstage == 2 ? d.C2 * d.C1 * d.k2 : 0;
    for (int i = threadIdx.x; i < nparams; i += kThreads) pacc[i] = 0.f;
    const float* xrow = xs + p * XP;
    float* xw = xs + p * XP;
    float* arow = a1s + p * AP;
    float* grow = gzs + p * AP;
    float* g2row = g2s + p * GP;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int b = grp / groups_per_sample, p0 = (grp % groups_per_sample) * PX;
        const int np = min(PX, d.N - p0);
        const int pix = p0 + p;
        const bool valid = p < np;
        __syncthreads();  // the previous group's tiles are done with
        load_tile<PX>(d, b, p0, np, CL, XP, xs);
        if (d.delta_mode != NPS_DECODE_NONE)
            for (int c = slot; c < d.num_c; c += NSLOT)
                uls[c * PX + p] = valid ? d.u[(((size_t)b * d.num_c + c) * d.tw + (d.tw - 1)) * d.N + pix] : 0.f;
        const float m = (d.mask && valid) ? d.mask[((size_t)b * d.mask_S + d.mask_ch) * d.N + pix] : 0.f;
        const float* gb = gout + (size_t)b * NT * d.N + pix;
        __syncthreads();
        // 1. stage 1: act and act' (one stage: times the gradient of its output, which is the chain's)
        for (int it = slot; it < A; it += NSLOT) {
            const int o = it / L1, t1 = it % L1;
            float a, da;
            act_both(d.act, d.beta, stage1(d, xrow, o, t1), a, da);
            if (d.nstage == 1) {
                const float g = valid ? gb[(size_t)it * d.N] : 0.f;
                da *= epilogue_grad(d, a, d.delta_mode != NPS_DECODE_NONE ? uls[o * PX + p] : 0.f, t1, m, g);
            }
            arow[it] = a;
            grow[it] = da;
        }
        if (d.nstage == 0) {  // the chain's output is the input: its gradient in place
            for (int it = slot; it < NT; it += NSLOT) {
                const int c = it / d.tw, t = it % d.tw;
                const float g = valid ? gb[(size_t)it * d.N] : 0.f;
                xw[it] = epilogue_grad(d, xrow[it], d.delta_mode != NPS_DECODE_NONE ? uls[c * PX + p] : 0.f, t, m, g);
            }
        }
        __syncthreads();
        if (d.nstage == 2) {
            // 2. stage 2 and the gradient of its output
            for (int it = slot; it < NT; it += NSLOT) {
                const int c = it / d.tw, t = it % d.tw;
                const float g = valid ? gb[(size_t)it * d.N] : 0.f;
                g2row[it] = epilogue_grad(d, stage2(d, arow, L1, c, t),
                                          d.delta_mode != NPS_DECODE_NONE ? uls[c * PX + p] : 0.f, t, m, g);
            }
            __syncthreads();
            // 3. parameter partials of stage 2: w2[o2][o][k], b2[o2]
            if (wants_p) {
                for (int it = slot; it < nw2 + d.C2; it += NSLOT) {
                    float s = 0.f;
                    if (it < nw2) {
                        const int o2 = it / (d.C1 * d.k2), o = (it / d.k2) % d.C1, k = it % d.k2;
                        const float* gr = g2row + o2 * d.tw;
                        const float* ar = arow + o * L1 + k;
                        for (int t = 0; t < d.tw; ++t) s = fmaf(gr[t], ar[t], s);
                    } else {
                        const float* gr = g2row + (it - nw2) * d.tw;
                        for (int t = 0; t < d.tw; ++t) s += gr[t];
                    }
                    s = pixel_sum<PX>(s);
                    if (p == 0) pacc[ow2 + it] += s;
                }
            }
            // 4. gradient of stage 1's pre-activation (in place over act')
            for (int it = slot; it < A; it += NSLOT) {
                const int o = it / L1, t1 = it % L1;
                const int klo = max(0, t1 - (d.tw - 1)), khi = min(d.k2 - 1, t1);
                float g = 0.f;
                for (int o2 = 0; o2 < d.C2; ++o2) {
                    const float* wr = d.w2 + (size_t)(o2 * d.C1 + o) * d.k2;
                    const float* gr = g2row + o2 * d.tw + t1;
                    for (int k = klo; k <= khi; ++k) g = fmaf(gr[-k], wr[k], g);
                }
                grow[it] *= g;
            }
            __syncthreads();
        }
        if (d.nstage >= 1) {
            // 5. parameter partials of stage 1: w1[o][ci][k], b1[o]
            if (wants_p) {
                for (int it = slot; it < nw1 + d.C1; it += NSLOT) {
                    float s = 0.f;
                    if (it < nw1) {
                        const int o = it / (d.C0 * d.k1), ci = (it / d.k1) % d.C0, k = it % d.k1;
                        const float* gr = grow + o * L1;
                        const float* xr = xrow + ci * d.L0 + k;
                        for (int t1 = 0; t1 < L1; ++t1) s = fmaf(gr[t1], xr[t1 * d.s1], s);
                    } else {
                        const float* gr = grow + (it - nw1) * L1;
                        for (int t1 = 0; t1 < L1; ++t1) s += gr[t1];
                    }
                    s = pixel_sum<PX>(s);
                    if (p == 0) pacc[it] += s;
                }
            }
            if (gx != nullptr) {
                __syncthreads();  // step 5 has read the input tile
                // 6. gradient of the input (in place over the tile): x[ci][j] feeds (o, t1) through tap k = j - t1 s1
                for (int it = slot; it < CL; it += NSLOT) {
                    const int ci = it / d.L0, j = it % d.L0;
                    const int tlo = max(0, (j - (d.k1 - 1) + d.s1 - 1) / d.s1), thi = min(L1 - 1, j / d.s1);
                    float g = 0.f;
                    for (int t1 = tlo; t1 <= thi; ++t1) {
                        const int k = j - t1 * d.s1;
                        for (int o = 0; o < d.C1; ++o) g = fmaf(grow[o * L1 + t1], d.w1[(size_t)(o * d.C0 + ci) * d.k1 + k], g);
                    }
                    xw[it] = g;
                }
            }
        }
        if (gx != nullptr) {
            __syncthreads();
            store_tile<PX>(d, gx, b, p0, np, CL, XP, xs);
        }
    }
    if (wants_p) {
        __syncthreads();
        for (int i = threadIdx.x; i < nparams; i += kThreads) ws[(size_t)blockIdx.x * nparams + i] = pacc[i];
    }
}

// out[c] = sum over rows of ws[row * pitch + c], rows taken in a fixed order: thread = (parameter, one of 4 row slices)
__global__ __launch_bounds__(kThreads) void decode_reduce_kernel(const float* __restrict__ ws, int rows, int pitch,
                                                                 int C, float* __restrict__ out) {
    __shared__ double part[kThreads];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), slice = threadIdx.x >> 6;
    double s = 0.0;
    if (c < C)
        for (int r = slice; r < rows; r += 4) s += (double)ws[(size_t)r * pitch + c];
    part[threadIdx.x] = s;
    __syncthreads();
    if (slice == 0 && c < C)
        out[c] = (float)(((part[threadIdx.x] + part[threadIdx.x + 64]) + part[threadIdx.x + 128]) +
                         part[threadIdx.x + 192]);
}

struct Plan {
    int L1, XP, AP, GP, nparams, px;
    size_t lds;
};

size_t lds_floats(const nps_decode_t* d, const Plan& pl, bool bwd, int px) {
    size_t f = (size_t)px * pl.XP + (size_t)d->num_c * px;
    if (!bwd) return f + (d->nstage == 2 ? (size_t)px * pl.AP : 0);
    if (d->nstage >= 1) f += 2 * (size_t)px * pl.AP;
    if (d->nstage == 2) f += (size_t)px * pl.GP;
    return f + pl.nparams;
}

// Host checks of a descriptor (no HIP call): sizes, pointers, and the LDS the chosen pixel group needs.
int decode_plan(const nps_decode_t* d, bool bwd, Plan* pl, const char* who) {
    NPS_CHECK_ARG(d != nullptr, "%s: NULL descriptor", who);
    NPS_CHECK_ARG(d->nstage >= 0 && d->nstage <= 2, "%s: nstage=%d (0, 1 or 2)", who, d->nstage);
    NPS_CHECK_ARG(d->B > 0 && d->N > 0 && d->C0 > 0 && d->L0 > 0 && d->num_c > 0 && d->tw > 0,
                  "%s: B=%d N=%d C0=%d L0=%d num_c=%d tw=%d must be positive", who, d->B, d->N, d->C0, d->L0,
                  d->num_c, d->tw);
    NPS_CHECK_ARG((long)d->C0 * d->L0 < (1L << 20) && (long)d->num_c * d->tw < (1L << 20),
                  "%s: C0*L0=%ld / num_c*tw=%ld too large", who, (long)d->C0 * d->L0, (long)d->num_c * d->tw);
    int Cf = d->C0, Lf = d->L0, L1 = 0;
    if (d->nstage >= 1) {
        NPS_CHECK_ARG(d->C1 > 0 && d->k1 > 0 && d->s1 > 0 && d->k1 <= d->L0,
                      "%s: stage 1 Conv1d(%d -> %d, k=%d, stride=%d) does not fit L0=%d", who, d->C0, d->C1, d->k1,
                      d->s1, d->L0);
        NPS_CHECK_ARG(d->act >= NPS_DECODE_ACT_NONE && d->act <= NPS_DECODE_ACT_SWISH,
                      "%s: act=%d (0 none, 1 GELU, 2 Swish)", who, d->act);
        NPS_CHECK_ARG(d->w1 && d->b1, "%s: stage 1 needs w1 and b1", who);
        L1 = (d->L0 - d->k1) / d->s1 + 1;
        Cf = d->C1;
        Lf = L1;
        NPS_CHECK_ARG((long)d->C1 * L1 < (1L << 20), "%s: C1*L1=%ld too large", who, (long)d->C1 * L1);
    }
    if (d->nstage == 2) {
        NPS_CHECK_ARG(d->C2 > 0 && d->k2 > 0 && d->k2 <= L1,
                      "%s: stage 2 Conv1d(%d -> %d, k=%d) does not fit L1=%d", who, d->C1, d->C2, d->k2, L1);
        NPS_CHECK_ARG(d->w2 && d->b2, "%s: stage 2 needs w2 and b2", who);
        Cf = d->C2;
        Lf = L1 - d->k2 + 1;
    }
    if (d->nstage == 0)
        NPS_CHECK_ARG((long)d->C0 * d->L0 == (long)d->num_c * d->tw,
                      "%s: no stages: C0*L0 = %d*%d is not num_c*tw = %d*%d", who, d->C0, d->L0, d->num_c, d->tw);
    else
        NPS_CHECK_ARG(Cf == d->num_c && Lf == d->tw,
                      "%s: the last stage yields %d channels x %d positions, not num_c=%d x tw=%d (C0=%d L0=%d C1=%d "
                      "k1=%d s1=%d C2=%d k2=%d)",
                      who, Cf, Lf, d->num_c, d->tw, d->C0, d->L0, d->C1, d->k1, d->s1, d->nstage == 2 ? d->C2 : 0,
                      d->nstage == 2 ? d->k2 : 0);
    NPS_CHECK_ARG(d->delta_mode >= NPS_DECODE_PER_STEP && d->delta_mode <= NPS_DECODE_NONE,
                  "%s: delta_mode=%d (0 per_step, 1 all, 2 none)", who, d->delta_mode);
    NPS_CHECK_ARG(d->delta_mode == NPS_DECODE_NONE || d->u, "%s: delta_mode=%d reads u", who, d->delta_mode);
    NPS_CHECK_ARG(d->delta_mode != NPS_DECODE_PER_STEP || d->dtcum, "%s: per_step needs dtcum", who);
    NPS_CHECK_ARG(!d->mask || (d->mask_ch >= 0 && d->mask_ch < d->mask_S), "%s: mask channel %d of %d", who,
                  d->mask_ch, d->mask_S);
    NPS_CHECK_ARG(d->x && (bwd || d->out), "%s: NULL x / out", who);
    NPS_CHECK_ARG(d->x_ps > 0 && d->x_cs > 0 && d->x_bs > 0, "%s: strides x_bs=%ld x_ps=%ld x_cs=%ld must be positive",
                  who, d->x_bs, d->x_ps, d->x_cs);
    NPS_CHECK_ARG(d->B <= 65535, "%s: B=%d exceeds the grid's y extent", who, d->B);
    pl->L1 = L1;
    pl->XP = (d->C0 * d->L0) | 1;
    pl->AP = d->nstage >= 1 ? (d->C1 * L1) | 1 : 1;
    pl->GP = (d->num_c * d->tw) | 1;
    pl->nparams = 0;
    if (d->nstage >= 1) pl->nparams += d->C1 * d->C0 * d->k1 + d->C1;
    if (d->nstage == 2) pl->nparams += d->C2 * d->C1 * d->k2 + d->C2;
    pl->px = 0;
    for (int px = 64; px >= 8; px >>= 1) {
        const size_t bytes = sizeof(float) * lds_floats(d, *pl, bwd, px);
        if (bytes <= kLdsBudget) {
            pl->px = px;
            pl->lds = bytes;
            break;
        }
    }
    NPS_CHECK_ARG(pl->px > 0,
                  "%s: 8 pixels of C0*L0=%d, C1*L1=%d, num_c*tw=%d do not fit %zu bytes of LDS", who, d->C0 * d->L0,
                  d->nstage >= 1 ? d->C1 * L1 : 0, d->num_c * d->tw, kLdsBudget);
    return 0;
}

int bwd_blocks(const nps_decode_t* d, const Plan& pl) {
    const long ngroups = (long)d->B * ((d->N + pl.px - 1) / pl.px);
    return (int)std::min<long>(ngroups, kBwdBlocks);
}

template <typename K>
void allow_lds(K kernel) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget);
}

}  // namespace

extern "C" int nps_decode_fwd(const nps_decode_t* d, void* stream) {
    Plan pl;
    if (int rc = decode_plan(d, false, &pl, "decode_fwd")) return rc;
    static bool attr_set = false;
    if (!attr_set) {
        allow_lds(decode_fwd_kernel<64>);
        allow_lds(decode_fwd_kernel<32>);
        allow_lds(decode_fwd_kernel<16>);
        allow_lds(decode_fwd_kernel<8>);
        attr_set = true;
    }
    const dim3 grid((d->N + pl.px - 1) / pl.px, d->B);
    hipStream_t s = (hipStream_t)stream;
    switch (pl.px) {
        case 64: decode_fwd_kernel<64><<<grid, kThreads, pl.lds, s>>>(*d, pl.L1, pl.XP, pl.AP); break;
        case 32: decode_fwd_kernel<32><<<grid, kThreads, pl.lds, s>>>(*d, pl.L1, pl.XP, pl.AP); break;
        case 16: decode_fwd_kernel<16><<<grid, kThreads, pl.lds, s>>>(*d, pl.L1, pl.XP, pl.AP); break;
        default: decode_fwd_kernel<8><<<grid, kThreads, pl.lds, s>>>(*d, pl.L1, pl.XP, pl.AP); break;
    }
    NPS_CHECK_LAUNCH("decode_fwd");
    return 0;
}

extern "C" size_t nps_decode_bwd_ws_floats(const nps_decode_t* d) {
    Plan pl;
    if (decode_plan(d, true, &pl, "decode_bwd_ws_floats")) return 0;
    return (size_t)bwd_blocks(d, pl) * pl.nparams;
}

extern "C" int nps_decode_bwd(const nps_decode_t* d, const float* gout, float* gx, float* gw1, float* gb1, float* gw2,
                              float* gb2, float* ws, void* stream) {
    Plan pl;
    if (int rc = decode_plan(d, true, &pl, "decode_bwd")) return rc;
    NPS_CHECK_ARG(gout != nullptr, "decode_bwd: NULL gout");
    const bool wants_p = (gw1 || gb1 || gw2 || gb2) && pl.nparams > 0;
    NPS_CHECK_ARG(d->nstage >= 1 || !(gw1 || gb1), "decode_bwd: gw1 / gb1 without a stage 1");
    NPS_CHECK_ARG(d->nstage == 2 || !(gw2 || gb2), "decode_bwd: gw2 / gb2 without a stage 2");
    NPS_CHECK_ARG(!wants_p || ws, "decode_bwd: parameter gradients need the workspace (nps_decode_bwd_ws_floats)");
    if (!gx && !wants_p) return 0;
    static bool attr_set = false;
    if (!attr_set) {
        allow_lds(decode_bwd_kernel<64>);
        allow_lds(decode_bwd_kernel<32>);
        allow_lds(decode_bwd_kernel<16>);
        allow_lds(decode_bwd_kernel<8>);
        attr_set = true;
    }
    const int gps = (d->N + pl.px - 1) / pl.px;
    NPS_CHECK_ARG((long)d->B * gps < (1L << 31), "decode_bwd: B=%d x N=%d pixel groups overflow", d->B, d->N);
    const int ngroups = d->B * gps;
    const int nblk = bwd_blocks(d, pl);
    float* wsp = wants_p ? ws : nullptr;
    hipStream_t s = (hipStream_t)stream;
#define NPS_DECODE_BWD(PXV)                                                                                        \
    decode_bwd_kernel<PXV><<<nblk, kThreads, pl.lds, s>>>(*d, gout, gx, wsp, pl.L1, pl.XP, pl.AP, pl.GP, pl.nparams, \
                                                          gps, ngroups)
    switch (pl.px) {
        case 64: NPS_DECODE_BWD(64); break;
        case 32: NPS_DECODE_BWD(32); break;
        case 16: NPS_DECODE_BWD(16); break;
        default: NPS_DECODE_BWD(8); break;
    }
#undef NPS_DECODE_BWD
    NPS_CHECK_LAUNCH("decode_bwd");
    if (wants_p) {
        // rows of ws -> the gradients the caller asked for; [w1 | b1 | w2 | b2] within a row
        const int nw1 = d->C1 * d->C0 * d->k1, nw2 = d->nstage == 2 ? d->C2 * d->C1 * d->k2 : 0;
        struct {
            float* out;
            int off, n;
        } parts[4] = {{gw1, 0, nw1}, {gb1, nw1, d->C1}, {gw2, nw1 + d->C1, nw2}, {gb2, nw1 + d->C1 + nw2, d->C2}};
        for (const auto& q : parts) {
            if (!q.out || q.n <= 0) continue;
            decode_reduce_kernel<<<(q.n + 63) / 64, kThreads, 0, s>>>(ws + q.off, nblk, pl.nparams, q.n, q.out);
            NPS_CHECK_LAUNCH("decode_bwd (reduce)");
        }
    }
    return 0;
}
