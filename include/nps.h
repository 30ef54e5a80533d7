/*
 * nps.h — C ABI of libnps_hip.so, the MI355X (gfx950) kernels behind the
 * neural-operator rollout hot path of yoeripoels/neural-pde-surrogates.
 *
 * The reference has no native code: every entry point below replaces the aten
 * calls that one reference Python site makes (cited per function, paths
 * relative to the reference's src/).  The drop-in boundary above this ABI is
 * the reference's own nn.Module / cfg surface, mirrored in
 * neural-pde-surrogates_amd/{models,trainers}.
 *
 * Conventions
 *  - Activations are fp32 NHWC ([B][H][W][C], C fastest) unless a field says
 *    otherwise; spectra are interleaved complex64 (float2).
 *  - All pointers are device pointers owned by the caller (PyTorch's caching
 *    allocator); the library never allocates.  `stream` is a hipStream_t
 *    (torch.cuda.current_stream().cuda_stream); every call is asynchronous
 *    and stream-ordered, never synchronises, and is hipGraph-capturable.
 *  - Return 0 on success, <0 on error (-1 bad argument / unsupported shape,
 *    -2 HIP launch error); nps_last_error() describes the last failure of the
 *    calling thread.
 */
#ifndef NPS_H
#define NPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPS_MAX_SRC 3

/* One channel-slice of a virtual (concatenated) conv input.
 * Replaces torch.cat along channels (proc_unet_modern.py:191, :351, :418;
 * proc_ufno.py:111; proc_dilatedresnet.py:49 [ref line 165]) and
 * crop_Nd's zero-pad/crop (models/common.py:20-34): the source tensor
 * [B][H][W][C] sits at (off_y, off_x) of the virtual input frame; frame
 * positions it does not cover read as 0 (before any normalisation). */
typedef struct {
    const float* ptr;
    int C, H, W;
    int off_y, off_x;
} nps_src_t;

/* Implicit-GEMM 2-D convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces nn.Conv2d / nn.ConvTranspose2d forward as built by
 * models/common.py:37-47, 93-120 (valid / zero / circular padding, stride,
 * dilation; a 4x4/s2 transposed conv is issued as 4 phase convs, see
 * DESIGN.md), with fused prologue GroupNorm+GELU (proc_unet_modern.py:245-247,
 * :194) and fused epilogue bias / addends / GELU / accumulate-at-offset
 * (the residual `crop_Nd(h) + shortcut` of proc_unet_modern.py:250, the
 * U-FNO sum+GELU of proc_ufno.py:118, the DRN residual of
 * proc_dilatedresnet.py:49). */
typedef struct {
    int nsrc;
    nps_src_t src[NPS_MAX_SRC];
    int B, Hin, Win, Cin;           /* virtual input frame; Cin = sum of src[i].C */
    /* prologue: x' = act(GN(x)) on every frame value (incl. crop zeros) */
    const double* gn_stats;         /* [B][G][2] = (sum, sum of squares) over the frame, or NULL */
    const float* gn_gamma;          /* [Cin] */
    const float* gn_beta;           /* [Cin] */
    int gn_groups;
    float gn_eps;
    int pre_act;                    /* 0 none, 1 GELU(erf) */
    /* geometry: input row for output row oy and tap ky is
     *   y_ext = oy*stride + ky*dil - pad_y  in a frame extended circularly by `circ`
     * on each side; y_ext outside [0, Hin+2*circ) reads 0 (after the prologue). */
    int KH, KW, stride, dil, pad_y, pad_x, circ;
    int Hout, Wout;
    const float* wpack;             /* nps_conv2d_pack_weights layout */
    const float* bias;              /* [Cout] or NULL */
    int Cout;
    /* epilogue: dest pixel = (oy*out_os + out_off_y, ox*out_os + out_off_x) */
    float* out;
    int out_C, out_H, out_W, out_os, out_off_y, out_off_x;
    int out_nchw;                   /* 1: out is [B][out_C][out_H][out_W] */
    int accumulate;                 /* out += result */
    const float* addend0;           /* indexed like out, or NULL */
    const float* addend1;
    int act;                        /* 0 none, 1 GELU */
    int add_after_act;              /* 0: act(acc+bias+addends); 1: act(acc+bias)+addends */
    /* tiling, chosen by nps_conv2d_plan() */
    int TH, TW, lattice, waves;
    /* arithmetic: NPS_PREC_F32 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32); NPS_PREC_X3F16 = 3-pass
     * split fp16 (x = hi + lo, products hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, fp32
     * accumulate, ~2^-21 relative per product; weights pre-scaled by an exact power of 2) — only where
     * nps_conv2d_x3_eligible() and nps_conv2d_x3_sources_ok(), with the weight packed by
     * nps_conv2d_pack_weights_x3 */
    int precision;
    /* Input range of a NPS_PREC_X3F16 conv.  The input is scaled by an exact power of 2 (max|x| into
     * [2^13, 2^14)) before the fp16 split and the result scaled back, so values of any magnitude keep
     * fp32-class accuracy (|x| >= max|x| * 2^-16 keep 22 bits; smaller ones an absolute error below
     * max|x| * 2^-37).  Each pointer is NULL or a RANGE TAG (NPS_TAG_FLOATS floats: NPS_TAG_SUB
     * sub-slots NPS_TAG_STRIDE floats apart, the tag's value is their max) holding an upper bound of
     * |x| over the source(s) it covers; the conv uses the max of the non-NULL tags, and scale 1 when
     * all three are NULL.  in_scale: set explicitly (nps_absmax of a gradient) or the tag of source 0;
     * in_tag1 / in_tag2: the tags of sources 1 / 2. */
    const float* in_scale;
    const float* in_tag1;
    const float* in_tag2;
    /* Range tag of the output (any precision, NULL = none): the conv raises it (atomic max of the
     * non-negative float bits, one sub-slot per wave) to >= max |value| of every element it writes.
     * Zero it before the first writer (tags are allocated from a zeroed arena, see ops.py). */
    float* out_tag;
    /* GroupNorm(1) moments of the output (NULL = none): [B][NPS_STATS_SUB][2] fp64 (sum, sum of squares;
     * the sample's moments are the sum over the sub-slots, which spread the atomics) to which the
     * conv ADDS, per sample, the moments of the values it stores — an accumulating conv the change of
     * the moments (stored value minus the value it replaced).  So a zeroed buffer after convs that write
     * every element of `out` once (a conv, the 4 phases of a transposed conv), or a buffer seeded with
     * `out`'s moments after an accumulating conv, holds what nps_group_norm_stats(G = 1) would compute
     * from `out`, without that pass.  Split-fp16 convs with NHWC output and Cout, out_C multiples of 4
     * only (1x1: Cout <= 192, bias-only epilogue); nps_conv2d_fwd refuses others. */
    double* out_stats;
    /* The 4 output phases of a k4/s2 ConvTranspose2d in ONE launch (split-fp16 2x2 convs; 0 or 1 = a single
     * conv): phase ph = 2 py + px uses the packed weight at wpack + ph * phase_wstride floats (its own
     * power-of-2 scale in its trailer) and writes at out_off + (py, px) (out_os = 2).  The phases share
     * the input patch: their work-groups are numbered phase-fastest on one XCD, so the patch is fetched
     * from HBM once (replaces 4 launches of the Upsample, common.py:93-120). */
    int nphase;
    long phase_wstride;
    /* Space-to-depth view (split-fp16 2x2 convs, one source, no prologue; 0 = off): the frame (Hin x Win x
     * Cin, Cin = 4 C) is the space-to-depth of src[0] (H x W x C, C % 16 == 0): frame pixel (y, x) channel
     * p C + c reads src[0] pixel (2 y + (p >> 1) - s2d_pad, 2 x + (p & 1) - s2d_pad) channel c, zero outside.
     * The U-Net Downsample's valid 3x3/s2 conv with padding s2d_pad (proc_unet_modern.py:439-455) runs as
     * a 2x2 stride-1 conv over this view (weight from nps_conv2d_pack_weights_x3 with transposed_phase = -2)
     * without materialising the space-to-depth copy. */
    int s2d;
    int s2d_pad;
    /* FNO layer fusion (1x1 split-fp16 convs on the LDS-weight kernel only; NULL = off): the truncated c2r W pass
     * of the spectral conv is added to the conv's result before the bias / act epilogue — out[b][y][x][o] =
     * act(w(x) + bias + spec_scale * sum_k c_k Re(spec_z[b][y][k][o] e^{2 pi i k x / W})), c_k = 2 except DC /
     * Nyquist (Im dropped), as nps_spectral_idft_w with accumulate (proc_fno.py:142-146: conv(x) + w(x)) — so the
     * separate idft_w read-modify-write of the output is gone.  spec_z: [B][Hout][spec_m2][Cout] complex64 (the
     * spectral pipeline's Z), Wout % 128 == 0, spec_m2 <= 16, no addend / accumulate. */
    const float* spec_z;
    int spec_m2;
    float spec_scale;
} nps_conv2d_t;

/* Range tags (nps_conv2d_t.in_scale / in_tag* / out_tag): 64 sub-slots 256 B apart, so the atomics of
 * thousands of work-groups spread over 64 addresses; readers take the max over the sub-slots. */
#define NPS_TAG_SUB 64
#define NPS_TAG_STRIDE 64
#define NPS_TAG_FLOATS (NPS_TAG_SUB * NPS_TAG_STRIDE)
/* sub-slots per sample of a moments buffer (nps_conv2d_t.out_stats) */
#ifndef NPS_STATS_SUB
#define NPS_STATS_SUB 16
#endif
int nps_stats_sub(void); /* NPS_STATS_SUB of this build (the moments buffers' sub-slot count) */

#define NPS_PREC_F32 0
#define NPS_PREC_X3F16 1

/* Floats of the packed weight buffer for a conv with the given shape
 * (ntaps = KH*KW). */
size_t nps_conv2d_packed_size(int Cout, int Cin, int ntaps);
/* Pack w[Cout][Cin][KH][KW] (nn.Conv2d layout, device pointer) into the
 * MFMA-fragment-native layout.  `transposed_phase` >= 0 packs the
 * stride-2 4x4 transposed-conv weight w[Cin][Cout][4][4]
 * (nn.ConvTranspose2d layout) as the 2x2 conv of output phase
 * (py, px) = (phase>>1, phase&1); KH = KW = 2 then.  transposed_phase == -2 packs a 3x3 stride-2
 * weight w[Cout][Cin/4][3][3] for the space-to-depth 2x2 form (KH = KW = 2, Cin = 4C).
 * transposed_phase == -3 packs the input-gradient conv of a stride-1 conv whose weight is
 * w[Cin][Cout][KH][KW] (Cout / Cin: the packed conv's): w transposed and flipped, element (co, ci, ky, kx) =
 * w[ci][co][KH-1-ky][KW-1-kx]. */
int nps_conv2d_pack_weights(const float* w, float* wpack, int Cout, int Cin, int KH, int KW,
                            int transposed_phase, void* stream);
/* Same transforms, packed as [hi | lo] fp16 MFMA fragments of s*w for precision = NPS_PREC_X3F16, with s
 * the power of 2 that maps max|w| into [2^13, 2^14) (max|w| is kept in the buffer's trailer; same buffer
 * size as nps_conv2d_packed_size).  1x1 weights are packed in 32-channel chunk pairs (each MFMA lane half
 * owns a contiguous 16-channel run), so the chunk count of a 1x1 packing is even. */
int nps_conv2d_pack_weights_x3(const float* w, float* wpack, int Cout, int Cin, int KH, int KW,
                               int transposed_phase, void* stream);
/* One weight of a batched split-fp16 packing: the arguments of nps_conv2d_pack_weights_x3. */
typedef struct {
    const float* w;
    float* wpack;
    int Cout, Cin, KH, KW;
    int transposed_phase;
} nps_pack_job_t;
/* n nps_conv2d_pack_weights_x3 calls (same results, bit for bit) in two launches per 48 jobs instead of two per job:
 * after an optimizer step every conv weight of the model is repacked (forward and input-gradient forms, trainers/
 * base.py:493 -> the next forward / backward), ~200 packings per U-FNO training step whose launch cost, not their
 * bytes, dominated.  jobs: a host array (copied into the launches' arguments). */
int nps_conv2d_pack_weights_x3_batch(const nps_pack_job_t* jobs, int n, void* stream);
/* 1 when a conv of this geometry runs on the split-fp16 kernel (stride-1: undilated 1x1 / 2x2 / 3x3, and
 * 5x5 at any dilation — the dilated ResNet's convs, proc_dilatedresnet.py:15-84). */
int nps_conv2d_x3_eligible(int KH, int KW, int stride, int dil);
/* 1 when the split-fp16 kernel applies a frame prologue itself (gn_groups > 0: GroupNorm affine with that
 * many groups; pre_act 1: GELU) — the 3x3 kernel, with Cin / gn_groups a multiple of 4 — so the caller
 * passes gn_* / pre_act to nps_conv2d_fwd instead of running nps_frame_pack first
 * (replaces ResidualBlock's norm -> act -> conv, proc_unet_modern.py:62-99). */
int nps_conv2d_x3_prologue_ok(int KH, int KW, int Cin, int gn_groups, int pre_act);
/* 1 when the split-fp16 kernel can stage this virtual frame directly: every source boundary on a
 * multiple of 16 channels, every source's C a multiple of 4 (otherwise nps_frame_pack it first). */
int nps_conv2d_x3_sources_ok(const nps_src_t* src, int nsrc);
/* Range tag `tag` (NPS_TAG_FLOATS floats) := max |x[i]| (zeroed, then raised) — the input range a
 * split-fp16 conv scales by (nps_conv2d_t.in_scale / in_tag*). */
int nps_absmax(const float* x, long n, float* tag, void* stream);
/* The same without the zeroing: raises `tag` (already zero, e.g. fresh from a zero-filled arena, or a valid lower
 * bound) to >= max |x[i]| — no memset launch. */
int nps_absmax_into(const float* x, long n, float* tag, void* stream);
/* Stride-2 3x3 convs (U-Net Downsample, proc_unet_modern.py:445-455) run as 2x2 stride-1 convs
 * over a space-to-depth copy: out[B][Hq][Wq][4C], channel (dy*2+dx)*C + c = x[2y+dy-pad][2x+dx-pad][c]
 * (zero outside); pack the weight with transposed_phase = -2 (Cin = 4C). */
int nps_space_to_depth(const float* x, float* out, int B, int H, int W, int C, int pad, int Hq, int Wq,
                       void* stream);
/* Fill TH/TW/lattice/waves of `a` for its shape; returns the LDS bytes used. */
int nps_conv2d_plan(nps_conv2d_t* a);
/* Highest byte (exclusive) of the packed split-fp16 weight that the launch of the planned *a reads (host-only
 * arithmetic of the kernel the launcher picks; must be <= 4 * nps_conv2d_packed_size).  Replaces no reference
 * interface: a check of this build's packing (tests/test_cabi.py). */
long nps_conv2d_x3_weight_span(const nps_conv2d_t* a);
int nps_conv2d_fwd(const nps_conv2d_t* a, void* stream);

/* Materialise a virtual frame: out[B][Hin][Win][Cin] = act(GN(frame)) using the prologue fields
 * of `a` (or the plain concat/crop when there is none); with a->out_C in (Cin, Cin + 4) the output
 * rows are out_C channels wide, the extra channels zero (4-channel alignment for the split-fp16 conv).  One HBM pass that evaluates the
 * GroupNorm affine + GELU once per element (proc_unet_modern.py:245-247) ahead of a conv that
 * then stages raw bytes only. */
int nps_frame_pack(const nps_conv2d_t* a, float* out, void* stream);

/* GroupNorm statistics over a virtual frame (same source semantics as the conv):
 * stats[B][G][2] += (sum, sumsq) in fp64.  Replaces the moments of
 * nn.GroupNorm (proc_unet_modern.py:235-236, :155).  stats must be zeroed
 * first (the call does it when zero_first != 0). */
int nps_group_norm_stats(const nps_src_t* src, int nsrc, int B, int Hin, int Win, int Cin, int G,
                         double* stats, int zero_first, void* stream);
/* Test hook: run the split-fp16 conv kernels on a persistent grid of `wgs` work-groups (> 0; 0 = one per
 * CU, the default) so every work-group walks many tiles. */
int nps_x3_set_grid(long wgs);

/* GroupNorm(1) moments of a virtual frame from those of its sources, each covering the frame exactly
 * (nps_conv2d_t.out_stats) — the per-source moments of torch.cat's GroupNorm (proc_unet_modern.py:235-236):
 * part i is [B][n_i][2] (n_i sub-slots; p1, p2 may be NULL), out is [B][n_out][2] and receives
 * out[b][0][k] = sum over parts and sub-slots of p_i[b][s][k] (its other sub-slots are left as they are). */
int nps_stats_sum(const double* p0, int n0, const double* p1, int n1, const double* p2, int n2, int B, double* out,
                  int n_out, void* stream);

/* ---- SpectralConv2d forward (proc_fno.py:257-288) ----------------------
 * Truncated DFTs replace rfft2 / irfft2: only the 2*m1 x m2 retained modes
 * are ever formed.  rows R = min(H, 2*m1) distinct retained k1 rows.
 *  X1[B][H][m2][C]    = sum_w x e^{-2pi i k2 w/W}          (nps_spectral_dft_w)
 *  X2[B][R][m2][C]    = sum_h X1 e^{-2pi i k1 h/H}          (nps_spectral_dft_h)
 *  Y [B][R][m2][Co]   = sum_i X2 * Wsel[i][o]               (nps_spectral_mix)
 *  Z [B][H][m2][Co]   = sum_r Y e^{+2pi i k1 h/H}           (nps_spectral_idft_h)
 *  y [B][H][W][Co]    = c2r_W(Z) / (H*W)  (+ epilogue)      (nps_spectral_idft_w)
 * c2r keeps Re of the DC (and Nyquist) bin only, as pocketfft/MKL do. */
int nps_spectral_dft_w(const nps_src_t* src, int nsrc, int B, int H, int W, int C, int m2,
                       float* X1, void* stream);
int nps_spectral_dft_h(const float* X1, float* X2, int B, int H, int m1, int m2, int C, void* stream);
/* wpack: [R][m2][Cin][Cout] complex — nps_spectral_pack_weights from the two
 * nn.Parameters weights1/weights2 [Cin][Cout][m1][m2] (complex64). */
int nps_spectral_pack_weights(const float* w1, const float* w2, float* wpack, int Cin, int Cout, int H,
                              int m1, int m2, void* stream);
int nps_spectral_mix(const float* X2, const float* wpack, float* Y, int B, int R, int m2, int Cin, int Cout,
                     void* stream);
int nps_spectral_idft_h(const float* Y, float* Z, int B, int H, int m1, int m2, int Cout, void* stream);
/* out[B][H][W][Cout] (= or +=) y ; optional addend, act as in nps_conv2d_t; out_tag (or NULL): the
 * output's range tag, raised to cover every value written (nps_conv2d_t.out_tag) */
int nps_spectral_idft_w(const float* Z, float* out, int B, int H, int W, int m2, int Cout, int accumulate,
                        const float* addend, int act, float* out_tag, void* stream);
/* The two W passes on channels-first activations (the reference modules' own layout): x / out are [B][C][H][W]
 * with W contiguous, plane stride H*W and a batch stride `*_bs` in elements (0 = dense, else >= C*H*W: a channel
 * slice of a larger NCHW tensor, e.g. one operand of a torch.cat, is passed as it lies).  NCDHW is the same view
 * with H = D*H.  Only 4-byte alignment is assumed.  X1 / Z keep the layouts above, so every stage between the W
 * passes is shared.  No addend and no range tag. */
int nps_spectral_dft_w_nchw(const float* x, long x_bs, int B, int H, int W, int C, int m2, float* X1, void* stream);
int nps_spectral_idft_w_nchw(const float* Z, float* out, long out_bs, int B, int H, int W, int m2, int Cout,
                             int accumulate, int act, void* stream);

/* ---- one call per module: SpectralConv2d / SpectralConv3d / FNO_Layer (composites of the stages) ------
 * The stage entry points above and below, sequenced inside the library, so a C caller runs a whole module
 * from this header alone.  x / y / dx: fp32 NHWC ([B][H][W][C]; 3-D: NDHWC, i.e. [B][D*H][W][C]); w1..w4 /
 * dw1..dw4: the modules' complex64 nn.Parameters in the reference layout ([Cin][Cout][m1][m2](+[m3]),
 * interleaved re/im), packed per call into the workspace; ws: caller-owned device memory of at least the
 * *_workspace() bytes (the same size serves forward and backward; 0 = bad shape).  No range tags or carried
 * moments: the plain reference semantics.  Errors: as every entry point (mode bounds as proc_fno.py:134-139). */
size_t nps_spectral_conv2d_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2);
/* SpectralConv2d.forward (proc_fno.py:257-288): y = irfft2(P(rfft2(x))) with accumulate = 0 (act = 0);
 * y = act(y + irfft2(...)) with accumulate = 1 (act 0 none / 1 GELU: FNO_Layer's sum + activation, :142-146). */
int nps_spectral_conv2d_fwd(const float* x, const float* w1, const float* w2, float* y, void* ws, int B, int Cin,
                            int Cout, int H, int W, int m1, int m2, int accumulate, int act, void* stream);
/* Its backward under torch.fft / complex-einsum autograd: dx = dL/dx (written; NULL = skip),
 * dw1 / dw2 = dL/dweights1, dL/dweights2 (written, PyTorch's conj(x) * g convention; both or neither). */
int nps_spectral_conv2d_bwd(const float* x, const float* w1, const float* w2, const float* dy, float* dx, float* dw1,
                            float* dw2, void* ws, int B, int Cin, int Cout, int H, int W, int m1, int m2,
                            void* stream);
/* FNO_Layer.forward (proc_fno.py:142-146, 2-D, conv_mode 'single'): w->out = act(SpectralConv2d(x) + w(x)).  `w`
 * is the layer's 1x1 conv `w`, filled in and nps_conv2d_plan()ned by the caller (src = the layer's input frame
 * covered by its sources, wpack, bias, out = y, act = the layer's activation, range tags), spec_z unset.  The
 * library picks the synthesis: fused into the 1x1's epilogue (nps_conv2d_t.spec_z: split-fp16, Wout % 128 == 0,
 * m2 <= 16, Cout <= 192, Cout % 4 == 0, no addend / accumulate), else the 1x1 then nps_spectral_idft_w
 * accumulating with the activation.  ws: nps_fno_layer2d_workspace bytes. */
size_t nps_fno_layer2d_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2);
int nps_fno_layer2d_fwd(const nps_conv2d_t* w, const float* w1, const float* w2, int m1, int m2, void* ws,
                        void* stream);
/* SpectralConv3d (proc_fno.py:291-376): the same pair over (D, H, W) with the four corner weights. */
size_t nps_spectral_conv3d_workspace(int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3);
int nps_spectral_conv3d_fwd(const float* x, const float* w1, const float* w2, const float* w3, const float* w4,
                            float* y, void* ws, int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3,
                            int accumulate, int act, void* stream);
int nps_spectral_conv3d_bwd(const float* x, const float* w1, const float* w2, const float* w3, const float* w4,
                            const float* dy, float* dx, float* dw1, float* dw2, float* dw3, float* dw4, void* ws,
                            int B, int Cin, int Cout, int D, int H, int W, int m1, int m2, int m3, void* stream);
/* The same four calls on the reference modules' own channels-first tensors: x / y / dy / dx are fp32 NCHW
 * ([B][C][H][W]; 3-D: NCDHW), each with a batch stride in elements (0 = dense, else >= C*H*W resp. C*D*H*W, so a
 * channel slice of a larger tensor needs no copy; a smaller or negative stride is an error).  Semantics, error
 * codes and mode bounds are those of the NHWC calls (dx == NULL skips dx, dw all or none).  The intermediates are
 * layout-independent, so nps_spectral_conv2d_workspace / nps_spectral_conv3d_workspace size `ws` for both
 * layouts.  y must not alias x (y is written while other rows of x are still being read). */
int nps_spectral_conv2d_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, float* y, long y_bs,
                                 void* ws, int B, int Cin, int Cout, int H, int W, int m1, int m2, int accumulate,
                                 int act, void* stream);
int nps_spectral_conv2d_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, const float* dy,
                                 long dy_bs, float* dx, long dx_bs, float* dw1, float* dw2, void* ws, int B, int Cin,
                                 int Cout, int H, int W, int m1, int m2, void* stream);
int nps_spectral_conv3d_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, const float* w3,
                                 const float* w4, float* y, long y_bs, void* ws, int B, int Cin, int Cout, int D, int H,
                                 int W, int m1, int m2, int m3, int accumulate, int act, void* stream);
int nps_spectral_conv3d_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, const float* w3,
                                 const float* w4, const float* dy, long dy_bs, float* dx, long dx_bs, float* dw1,
                                 float* dw2, float* dw3, float* dw4, void* ws, int B, int Cin, int Cout, int D, int H,
                                 int W, int m1, int m2, int m3, void* stream);

/* ---- FiLM conditioning of SpectralConv2d (proc_fno.py:271-284, cond_mode "film") ----------------------
 * The retained modes are multiplied by a real per-sample, per-channel, per-mode factor from the module's
 * weights_feat = nn.Linear(K, N), N = Cout*2*m1*m2, applied to the conditioning vector p:
 *  p [B][K] fp32, wf = weights_feat.weight [N][K], bias = weights_feat.bias [N],
 *  F[b][n] = bias[n] + sum_k p[b][k] wf[n][k],  n(o, j, k2) = (o*2*m1 + j)*m2 + k2  (.view(B, Cout, 2*m1, m2)).
 * Row j < m1 of F sits on frequency k1 = j (the [:m1] corner, "low"), row j >= m1 on k1 = H - 2*m1 + j (the
 * [-m1:] corner, "high"); with 2*m1 > H a frequency can be both.
 *  S [B][R][m2][Cout] real, the layout of Y:
 *   transform_mode 0: S = 1 + [low] F(j_lo) + [high] F(j_hi)   (both terms where the corners overlap)
 *   transform_mode 1: S = F(j_hi) if high, else F(j_lo)        (the second write wins, as for the weights)
 * Errors (-1, text in nps_last_error): K outside [1, 64], transform_mode not 0 / 1, m1 > H, R > 32. */
int nps_spectral_film_scale(const float* p, const float* wf, const float* bias, float* S, int B, int K, int Cout,
                            int H, int m1, int m2, int transform_mode, void* stream);
/* nps_spectral_mix with Y[b][r][k2][o] multiplied by S[b][r][k2][o] in the mixer's store (same kernels, same
 * dispatch; S == 1 gives nps_spectral_mix's bits) */
int nps_spectral_mix_scaled(const float* X2, const float* wpack, const float* S, float* Y, int B, int R, int m2,
                            int Cin, int Cout, void* stream);
/* Backward of Ys = Y * S.  Y [B][R][m2][Cout] complex: the UNSCALED mixer output (nps_spectral_mix of the saved X2;
 * never Ys / S, S may be zero); g: the gradient arriving at Ys (PyTorch's convention), replaced in place by
 * g * S = the gradient of Y; gS [B][R][m2][Cout] real (written) = Re Y Re g + Im Y Im g. */
int nps_spectral_film_bwd(const float* Y, const float* S, float* g, float* gS, int B, int R, int m2, int Cout,
                          void* stream);
/* Gradients of the linear layer from gS, each output written or NULL = skipped: gwf [N][K] = sum_b gF[b][n] p[b][k],
 * gbias [N] = sum_b gF[b][n], gp [B][K] = sum_n gF[b][n] wf[n][k], with gF[b][n(o, j, k2)] = gS[b][row(j)][k2][o]
 * (zero, in transform_mode 1, for the rows j < m1 that the [-m1:] corner overwrote).  fp64 sums in a fixed order,
 * no atomics: bit-repeatable. */
int nps_spectral_film_param_bwd(const float* gS, const float* p, const float* wf, float* gwf, float* gbias, float* gp,
                                int B, int K, int Cout, int H, int m1, int m2, int transform_mode, void* stream);
/* The one-call composites with FiLM: nps_spectral_conv2d_fwd / _bwd and their channels-first forms with the
 * operands p, wf, bias, K, transform_mode added (layouts, batch strides, accumulate / act, dx == NULL, dw1 / dw2
 * both or neither as there); dp [B][K], dwf [N][K], dbias [N]: written, each NULL = skipped.  `ws` holds at least
 * nps_spectral_conv2d_film_workspace() bytes (the plain workspace plus S, the unscaled Y and gS). */
size_t nps_spectral_conv2d_film_workspace(int B, int Cin, int Cout, int H, int W, int m1, int m2);
int nps_spectral_conv2d_film_fwd(const float* x, const float* w1, const float* w2, const float* p, const float* wf,
                                 const float* bias, float* y, void* ws, int B, int Cin, int Cout, int H, int W,
                                 int m1, int m2, int K, int transform_mode, int accumulate, int act, void* stream);
int nps_spectral_conv2d_film_bwd(const float* x, const float* w1, const float* w2, const float* p, const float* wf,
                                 const float* bias, const float* dy, float* dx, float* dw1, float* dw2, float* dp,
                                 float* dwf, float* dbias, void* ws, int B, int Cin, int Cout, int H, int W, int m1,
                                 int m2, int K, int transform_mode, void* stream);
int nps_spectral_conv2d_film_fwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, const float* p,
                                      const float* wf, const float* bias, float* y, long y_bs, void* ws, int B,
                                      int Cin, int Cout, int H, int W, int m1, int m2, int K, int transform_mode,
                                      int accumulate, int act, void* stream);
int nps_spectral_conv2d_film_bwd_nchw(const float* x, long x_bs, const float* w1, const float* w2, const float* p,
                                      const float* wf, const float* bias, const float* dy, long dy_bs, float* dx,
                                      long dx_bs, float* dw1, float* dw2, float* dp, float* dwf, float* dbias,
                                      void* ws, int B, int Cin, int Cout, int H, int W, int m1, int m2, int K,
                                      int transform_mode, void* stream);

/* ---- SpectralConv1d / FNO-1D (proc_fno.py:158-222) ----------------------------------------------------
 * Channels-last activations (B, L, C); weights1 [Cin][Cout][m] complex64; m <= L / 2 + 1.
 *  X[B][m][C]   = sum_l x e^{-2 pi i k l / L}                     (nps_spectral1d_dft)
 *  Y[B][m][Co]  = sum_i X * W[i][o][k]  (* S with FiLM)            (nps_spectral_mix / _mix_scaled, R = 1, m2 = m)
 *  y[B][L][Co]  = c2r_L(Y) / L  (+ epilogue)                       (nps_spectral1d_idft)
 * Both transforms split L over work-groups; the analysis adds a work-group's sub-chunks in ascending order in
 * LDS and the work-groups' partials in ascending order in a second kernel (no atomics: bit-repeatable).  Envelope: 1 <= B <= 65535, C >= 1, 2 <= L <= 65536,
 * 1 <= m <= min(L / 2 + 1, 128); anything else is an error (-1, text in nps_last_error) before any launch.
 *
 * dft: `src` as for nps_spectral_dft_w with H = 1, W = L (up to NPS_MAX_SRC sources, any channel counts; 16-B
 * loads when every source has C % 4 == 0); ws: nps_spectral1d_dft_workspace(B, L, C, m) bytes of device memory
 * (0 = bad shape) for the partials.  adjoint != 0: every bin scaled by c_k / L (c_k = 1 for DC and the Nyquist
 * bin of an even L, else 2), the adjoint of nps_spectral1d_idft's synthesis (gy -> gY). */
size_t nps_spectral1d_dft_workspace(int B, int L, int C, int m);
int nps_spectral1d_dft(const nps_src_t* src, int nsrc, int B, int L, int C, int m, float* X, float* ws, int adjoint,
                       void* stream);
/* idft: out[B][L][Cout] (= or +=) act(y + addend), accumulate / addend / act as for nps_spectral_idft_w.
 * adjoint != 0: no doubling and no 1 / L, gx[l] = sum_k Re(gX_k e^{+2 pi i k l / L}), the adjoint of the analysis. */
int nps_spectral1d_idft(const float* Z, float* out, int B, int L, int m, int Cout, int accumulate, const float* addend,
                        int act, int adjoint, void* stream);
/* wpack [m][Cin][Cout] complex (the mixer's layout with R = 1) from weights1 [Cin][Cout][m], and the adjoint */
int nps_spectral1d_pack_weights(const float* w, float* wpack, int Cin, int Cout, int m, void* stream);
int nps_spectral1d_unpack_grad(const float* gwpack, float* gw, int Cin, int Cout, int m, void* stream);
/* nps_spectral_mix_bwd (R = 1, m2 = m) at any batch size: runs of 32 samples, each run's weight gradient into its
 * own part of gwpack [nps_spectral1d_mix_bwd_parts(B)][m][Cin][Cout], then the parts added into part 0 in ascending
 * order (the result; the other parts are scratch). */
int nps_spectral1d_mix_bwd_parts(int B);
int nps_spectral1d_mix_bwd(const float* X, const float* wpack, const float* gY, float* gX, float* gwpack, int B, int m,
                           int Cin, int Cout, void* stream);
/* FiLM (proc_fno.py:209-218): F[b][n] = bias[n] + sum_k p[b][k] wf[n][k], n = o * m + k (.view(B, Cout, m), no
 * factor 2); S[B][m][Cout] = 1 + F (transform_mode 0) or F (1).  K in [1, 64].  nps_spectral_film_bwd (R = 1) gives
 * gS; param_bwd: gwf [N][K], gbias [N], gp [B][K], each written or NULL = skipped, fp64 sums in a fixed order. */
int nps_spectral1d_film_scale(const float* p, const float* wf, const float* bias, float* S, int B, int K, int Cout,
                              int m, int transform_mode, void* stream);
int nps_spectral1d_film_param_bwd(const float* gS, const float* p, const float* wf, float* gwf, float* gbias,
                                  float* gp, int B, int K, int Cout, int m, int transform_mode, void* stream);
/* One call per module, as nps_spectral_conv2d_*: x / y / dy / dx fp32 [B][L][C], w / dw the complex64 nn.Parameter
 * [Cin][Cout][m], ws >= the *_workspace() bytes (forward and backward alike; 0 = bad shape); dx, dw, dp, dwf,
 * dbias: written, each NULL = skipped. */
size_t nps_spectral_conv1d_workspace(int B, int Cin, int Cout, int L, int m);
int nps_spectral_conv1d_fwd(const float* x, const float* w, float* y, void* ws, int B, int Cin, int Cout, int L, int m,
                            int accumulate, int act, void* stream);
int nps_spectral_conv1d_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, void* ws, int B,
                            int Cin, int Cout, int L, int m, void* stream);
size_t nps_spectral_conv1d_film_workspace(int B, int Cin, int Cout, int L, int m);
int nps_spectral_conv1d_film_fwd(const float* x, const float* w, const float* p, const float* wf, const float* bias,
                                 float* y, void* ws, int B, int Cin, int Cout, int L, int m, int K, int transform_mode,
                                 int accumulate, int act, void* stream);
int nps_spectral_conv1d_film_bwd(const float* x, const float* w, const float* p, const float* wf, const float* bias,
                                 const float* dy, float* dx, float* dw, float* dp, float* dwf, float* dbias, void* ws,
                                 int B, int Cin, int Cout, int L, int m, int K, int transform_mode, void* stream);

/* ---- bf16 storage (BASELINE config C5: the 3-D rFFT spectral conv in bf16) ----------------------------
 * Activations in HBM as bf16 (16-bit storage of NDHWC tensors viewed as (B, D*H, W, C)), every sum in fp32:
 * the same transforms as the fp32 entry points above.  Replaces the fp32 SpectralConv3d / FNO_Layer chain of
 * proc_fno.py:291-376, :142-146 for a bf16 model (the reference has no bf16 path: CPU FFT rejects bf16,
 * SURVEY.md §0.5); parity is checked against the fp32 HIP path, itself pinned to the oracle. */
int nps_spectral_dft_w_bf16(const nps_src_t* src, int nsrc, int B, int H, int W, int C, int m2, float* X1,
                            void* stream);
/* wpack: the nps_spectral(3d)_pack_weights layout with every complex value as a packed bf16 (re, im) pair
 * (nps_f32_to_bf16 of the fp32 packing) */
int nps_spectral_mix_bf16(const float* X2, const void* wpack, float* Y, int B, int R, int m2, int Cin, int Cout,
                          void* stream);
/* out / addend bf16 [B][H][W][Cout]; out (= or +=) act(c2r(Z)/(H W) + addend).  The bins are summed 16 at a time and
 * the running sum lives in `out` between chunks: for m2 <= 16 (C5: m3 = 12) the fp32 sum is rounded to bf16 once, at
 * the store; for m2 > 16 the partial sums are also rounded to bf16, once per extra chunk (the partial over the first
 * 16 j bins, j = 1, 2, ..., adds up to 2^-8 of its magnitude to the error of the result;
 * tests/test_gpu_bf16_stages.py). */
int nps_spectral_idft_w_bf16(const float* Z, void* out, int B, int H, int W, int m2, int Cout, int accumulate,
                             const void* addend, int act, void* stream);
/* elementwise conversion (bf16 round-to-nearest-even) */
int nps_f32_to_bf16(const float* x, long n, void* y, void* stream);
int nps_bf16_to_f32(const void* x, long n, float* y, void* stream);
/* pointwise conv (FNO_Layer `w` with kernel 1, proc_fno.py:104-107) in bf16: a->src / a->out / a->addend0 bf16
 * NHWC (sources covering the frame, all but the last with C % 8 == 0), a->wpack from nps_pack_1x1_bf16
 * ([Cout][nps_conv1x1_bf16_kr(Cin)] bf16), a->bias fp32, epilogue act(acc + bias + addend0) on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; Cout in {32, 64, 96, 128, 192, 256}. */
int nps_conv1x1_bf16_kr(int Cin);
int nps_pack_1x1_bf16(const float* w, void* wp, int Cout, int Cin, void* stream);
int nps_conv1x1_bf16(const nps_conv2d_t* a, void* stream);

/* ---- grid encoder / decoder / wrapper ---------------------------------
 * Encoder input packing, enc_grid.py:41-50 + enc_proc_dec.py:127-137:
 * xin[B][H][W][Cp] = [u(B,c,tw,H,W) flattened c*tw | pos(B,H,W,2) | cond(B,K) broadcast | sc(B,S,H,W)],
 * zero-padded to Cp channels; vb[B][H][W][K+S] = [cond broadcast | sc]. */
int nps_pack_grid_input(const float* u, const float* pos, const float* cond, const float* sc, float* xin,
                        float* vb, int B, int CT, int H, int W, int K, int S, int Cp, void* stream);
/* The same packing on a grid of any dimension, over N = the product of the spatial extents (L, H*W, D*H*W) flat
 * pixels: u planar [B][CT][N], pos [B][N][P], cond [B][K], sc [B][S][N] ->
 * xin[B][N][Cp] = [u | pos(P) | cond(K) broadcast | sc(S) | 0-pad], vb[B][N][K+S] = [cond broadcast | sc] (vb may be
 * NULL when K + S == 0).  P, the number of position channels, is the grid's dimension: 1, 2 or 3 (anything else is
 * an error); Cp % 4 == 0, Cp >= CT + P + K + S, 260 * Cp bytes of LDS <= 64 KiB.  nps_pack_grid_input is this with
 * N = H * W, P = 2. */
int nps_pack_grid_input_nd(const float* u, const float* pos, const float* cond, const float* sc, float* xin,
                           float* vb, int B, int CT, int N, int P, int K, int S, int Cp, void* stream);
/* TimeConvDense conv1d chain + add_delta + tanh + spatial-cond mask
 * (dec_grid.py:126-146, :8-31; activation_wrapper.py:34-35).
 * pre: [B][num_c*3*tw][H][W] (planar pre_decoder output), u: model input
 * (B,num_c,tw,H,W); out: (B,num_c,tw,H,W).  dtcum[tw] = fp32 cumsum(dt).
 * mask: (B,S,H,W) channel `mask_ch` or NULL.  The chain is per pixel and the kernels index by H * W only: a 1-D or
 * 3-D grid passes its flat pixel count as H = 1, W = N (nps_timeconv_decode_bwd likewise). */
int nps_timeconv_decode(const float* pre, const float* u, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* dtcum, const float* mask, int mask_S, int mask_ch,
                        float* out, int B, int num_c, int tw, int H, int W, int act_tanh, void* stream);
/* sums[p] = sum over plane p (plane_size floats at base + p*plane_stride), fp64 */
int nps_plane_sums(const float* base, long plane_stride, int plane_size, int nplanes, double* sums,
                   void* stream);
/* approx_volume_preserve 'individual_static' rescale + mask (activation_wrapper.py:80-105), in place.
 * new_tot[B*c*tw], prev_tot[B*c] (fp64 sums); mpdcum[tw] = fp32 cumsum(max_pct_dif). */
int nps_volume_rescale(float* u, const double* new_tot, const double* prev_tot, const float* mpdcum,
                       const float* mask, int mask_S, int mask_ch, int B, int num_c, int tw, int H, int W,
                       void* stream);
/* MSE_sum between two equal-size tensors, fp64: *out += sum((a-b)^2)  (nn.MSELoss(reduction='sum')) */
int nps_sq_err_sum(const float* a, const float* b, long n, double* out, void* stream);
/* layout transforms at module boundaries */
int nps_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, void* stream);
int nps_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, void* stream);

/* ==== backward (training) ================================================
 * The pushforward train_step (trainers/autoregressivepushforwardtrainer.py:43-163) and
 * trainers/base.py:492 `loss.backward()` differentiate every op above.  Input gradients of a
 * conv are forward convs of dy (nps_conv2d_fwd) with flipped / transposed / phase-split weights;
 * the entries below provide the rest. */

/* Weight gradient of a stride-1 (optionally dilated, zero- or circularly-padded) conv on fp32
 * MFMA: g[m][n][ky*KW + kx] += sum_{b,py,px} a[b][py][px][m] * X[b][y][x][n] with
 * (y, x) = (py + ky*dil - pad_y, px + kx*dil - pad_x) in the frame extended circularly by
 * `circ` (outside it reads 0) — the same geometry as nps_conv2d_t.  For a conv, a = dy and
 * X = its input, so g is the nn.Conv2d weight grad [Cout][Cin][KH][KW]; stride-2 and transposed
 * convs are issued in their space-to-depth / phase form.  Replaces aten
 * convolution_backward's weight output for models/common.py:37-47, 93-120. */
typedef struct {
    const float* a;                 /* [B][Ha][Wa][M] (NHWC) */
    int B, Ha, Wa, M;
    const float* x;                 /* [B][Hx][Wx][N] (NHWC) */
    int Hx, Wx, N;
    int KH, KW, dil, pad_y, pad_x, circ;
    float* g;                       /* [M][N][KH*KW], accumulated with += */
    /* [M] or NULL: the split-fp16 entry points (nps_conv2d_wgrad_x3 / _set) also give db[m] = sum_{b,py,px}
     * a[b][py][px][m] — the conv's bias gradient when a = dy — with g's semantics (+= / =), from the values the
     * kernel stages anyway (no nps_channel_sums pass over dy).  Must be NULL for nps_conv2d_wgrad. */
    float* db;
} nps_wgrad_t;
size_t nps_wgrad_lds_bytes(int KH, int KW);
int nps_conv2d_wgrad(const nps_wgrad_t* p, void* stream);
/* The same weight gradient in the split-fp16 arithmetic of NPS_PREC_X3F16 (3 fp16 MFMA products per
 * fp32 product, fp32 accumulation) for undilated 1x1 / 2x2 / 3x3 kernels (KH == KW) over channel
 * counts M, N that are multiples of 4: a and x are scaled by exact powers of two from their range tags
 * a_range / x_range (NPS_TAG_FLOATS floats, e.g. from nps_absmax) before the split.  ws: a device
 * workspace of nps_wgrad_x3_ws_floats(M, N, KH, KW) floats (the split-K partials accumulate there
 * tap-major, then fold into g).  Same geometry and += semantics as nps_conv2d_wgrad. */
size_t nps_wgrad_x3_ws_floats(int M, int N, int KH, int KW);  /* KH*KW*M*N partials + M (the bias row) */
int nps_conv2d_wgrad_x3(const nps_wgrad_t* p, const float* a_range, const float* x_range, float* ws, void* stream);
/* The same, storing G = the weight gradient (g need not be zeroed beforehand) instead of adding to it. */
int nps_conv2d_wgrad_x3_set(const nps_wgrad_t* p, const float* a_range, const float* x_range, float* ws,
                            void* stream);
/* Test hook (host code only, launches nothing): the launch plan nps_conv2d_wgrad_x3 would use for *p.
 * out[0] kernel (0: wgrad_x3_kernel<KH,KW>, 1: wgrad1_wide_kernel, 2: wgrad2_wide_kernel), out[1] ntiles,
 * out[2] base (m x n tiles), out[3] n_nt, out[4] splits, out[5] tiles per split, out[6] remap, out[7] grid.
 * < 0 where nps_conv2d_wgrad_x3 would refuse p. */
int nps_conv2d_wgrad_x3_plan(const nps_wgrad_t* p, int out[8]);
/* out[c] += sum over `rows` rows of x[row][c] (conv bias gradients; parameter-partial reductions) */
int nps_channel_sums(const float* x, long rows, int C, float* out, void* stream);

/* Backward of nps_frame_pack: torch.cat + crop_Nd + GroupNorm + GELU (proc_unet_modern.py:245-247,
 * :194, common.py:20-34) given gy = dL/d(frame).  dsrc[i] (shape of source i, or NULL) receives the
 * gradient of each source (0 where the source lies outside the frame); dgamma/dbeta [Cin] are written
 * when the prologue has a GroupNorm; work = [B][2][Cin] fp64 scratch. */
int nps_frame_pack_bwd(const nps_conv2d_t* a, const float* gy, float* const* dsrc, float* dgamma, float* dbeta,
                       double* work, void* stream);
/* The same, also raising the range tag dtag[i] (NPS_TAG_FLOATS floats, or NULL; dtag itself may be NULL) to
 * cover |dsrc[i]| — the range of the gradient the next conv backward reads as its dy. */
int nps_frame_pack_bwd_tagged(const nps_conv2d_t* a, const float* gy, float* const* dsrc, float* const* dtag,
                              float* dgamma, float* dbeta, double* work, void* stream);
/* The same with gy_plain (or NULL): the gradient of the plain concatenation of the same sources (the frame without
 * prologue, shaped like gy) from a second consumer — the ResidualBlock's shortcut conv or identity path
 * (proc_unet_modern.py:243-250) — added into dsrc in the same pass instead of by a separate accumulation.
 * Unlike the two above, `work` must hold zeros on entry (e.g. a slice of a zero-filled buffer used once): no
 * memset launch per frame. */
int nps_frame_pack_bwd2(const nps_conv2d_t* a, const float* gy, const float* gy_plain, float* const* dsrc,
                        float* const* dtag, float* dgamma, float* dbeta, double* work, void* stream);

/* element-wise pieces of the differentiated graph */
int nps_gelu(const float* x, float* y, long n, void* stream);                                /* nn.GELU() */
int nps_gelu_bwd(const float* x, const float* gy, float* gx, long n, void* stream);
/* out[b][y+off_y][x+off_x][c] += src[b][y][x][c] (crop_Nd(h) + shortcut, proc_unet_modern.py:250) */
int nps_add_at(float* out, const float* src, int B, int Ho, int Wo, int Hs, int Ws, int C, int off_y, int off_x,
               void* stream);
/* out = base + that placement of src, in one pass (out, base: [B][Ho][Wo][C]; C % 4 == 0, 16-B aligned);
   out_stats: NULL, or [B][NPS_STATS_SUB][2] fp64 to which the launch ADDS out's GroupNorm(1) moments (sum, sum of
   squares per sample), as nps_conv2d_t.out_stats */
int nps_add_at_copy(float* out, const float* base, const float* src, int B, int Ho, int Wo, int Hs, int Ws, int C,
                    int off_y, int off_x, double* out_stats, void* stream);
/* circular_pad_2d (models/common.py:61-90) on NHWC and its adjoint (wrap-sum) */
int nps_circular_pad(const float* x, float* out, int B, int H, int W, int C, int pad, void* stream);
int nps_circular_fold(const float* gp, float* gx, int B, int H, int W, int C, int pad, void* stream);
/* out = (*scale) * (a - b): gradient of sqrt(MSELoss(sum)) (autoregressivepushforwardtrainer.py:158-162) */
int nps_scaled_diff(const float* a, const float* b, const double* scale, float* out, long n, void* stream);

/* SpectralConv2d backward (proc_fno.py:257-288 under torch.fft autograd):
 *  gZ  = (c_k / (H W)) DFT_W(gy)  on the m2 kept bins (c_k = 1 for DC/Nyquist, else 2)  idft_w_bwd
 *  gY  = nps_spectral_dft_h(gZ);   gX2, gwpack = mix_bwd(X2, wpack, gY)
 *  gX1 = nps_spectral_idft_h(gX2); gx[w] = sum_k Re(gX1[k] e^{+2 pi i k w / W})           dft_w_bwd
 *  gweights1/2 = unpack_grad(gwpack)  (PyTorch's complex-gradient convention, conj(x) * g) */
int nps_spectral_idft_w_bwd(const float* gy, float* gZ, int B, int H, int W, int m2, int Cout, void* stream);
int nps_spectral_dft_w_bwd(const float* gX1, float* gx, int B, int H, int W, int m2, int Cin, void* stream);
/* the same two adjoint W passes reading gy / writing gx channels-first (layout and batch stride as
 * nps_spectral_dft_w_nchw) */
int nps_spectral_idft_w_bwd_nchw(const float* gy, long gy_bs, float* gZ, int B, int H, int W, int m2, int Cout,
                                 void* stream);
int nps_spectral_dft_w_bwd_nchw(const float* gX1, float* gx, long gx_bs, int B, int H, int W, int m2, int Cin,
                                void* stream);
int nps_spectral_mix_bwd(const float* X2, const float* wpack, const float* gY, float* gX2, float* gwpack, int B,
                         int R, int m2, int Cin, int Cout, void* stream);
int nps_spectral_unpack_grad(const float* gwpack, float* gw1, float* gw2, int Cin, int Cout, int H, int m1, int m2,
                             void* stream);

/* SpectralConv3d (proc_fno.py:291-376: rfftn over (D, H, W) -> 4 retained corners weights1..4 -> irfftn)
 * on NDHWC activations, composed of the 2-D stages above applied per axis:
 *  W: dft_w over (B, D*H, W)                 -> X1 [B][D*H][m3][C]
 *  H: dft_h over (B*D, H), m2 := m3          -> X2 [B*D][R2][m3][C]        R2 = min(H, 2*m2)
 *  D: dft_h over (B, D),   m2 := R2*m3       -> X3 [B][R1][R2*m3][C]       R1 = min(D, 2*m1)
 *  mix(X3, wpack, R := R1, m2 := R2*m3); idft_h (D), idft_h (H), idft_w over (B, D*H, W) (1/(D*H*W)).
 * The backward is the same adjoint chain as the 2-D one, axis by axis.
 * wpack: [R1][R2][m3][Cin][Cout] complex; where corners overlap the later reference write wins
 * (w1 [:m1,:m2] < w2 [-m1:,:m2] < w3 [:m1,-m2:] < w4 [-m1:,-m2:], proc_fno.py:342-350). */
int nps_spectral3d_pack_weights(const float* w1, const float* w2, const float* w3, const float* w4, float* wpack,
                                int Cin, int Cout, int D, int H, int m1, int m2, int m3, void* stream);
/* gweights1..4 [Cin][Cout][m1][m2][m3] from gwpack (0 where a later corner owns the mode) */
int nps_spectral3d_unpack_grad(const float* gwpack, float* gw1, float* gw2, float* gw3, float* gw4, int Cin, int Cout,
                               int D, int H, int m1, int m2, int m3, void* stream);

/* TimeConvDense + add_delta + tanh + mask backward (dec_grid.py:126-146, :8-31): gpre is planar like
 * `pre`; ws[blocks][params] receives per-block partials of [w1 | b1 | w2 | b2] (blocks = B*ceil(H*W/64),
 * params = 2c*c*ka + 2c + c*2c*kb + c), reduced with nps_channel_sums. */
int nps_timeconv_decode_bwd(const float* pre, const float* u, const float* w1, const float* b1, const float* w2,
                            const float* b2, const float* dtcum, const float* mask, int mask_S, int mask_ch,
                            const float* gout, float* gpre, float* ws, int B, int num_c, int tw, int H, int W,
                            int act_tanh, void* stream);
/* 'individual_static' volume rescale backward (activation_wrapper.py:80-105):
 * D[plane] = sum g (1 - m) u_in (nps_plane_dot), then gu_in (nps_volume_rescale_bwd). */
int nps_plane_dot(const float* g, const float* u, const float* mask, int mask_S, int mask_ch, int B, int nct, int H,
                  int W, double* D, void* stream);
int nps_volume_rescale_bwd(const float* g, const double* new_tot, const double* prev_tot, const float* mpdcum,
                           const float* mask, int mask_S, int mask_ch, const double* D, float* gu, int B, int num_c,
                           int tw, int H, int W, void* stream);

/* ---- approx_volume_preserve 'block' and 'individual' (csrc/volume.hip; activation_wrapper.py:40-79) ----
 * With s_t = sum_hw u[b,c,t] and p = sum_hw x[b,c,-1] (new_tot[B*c*tw], prev_tot[B*c]: nps_plane_sums), m =
 * max_pct_dif and r(s, p) = 1 - tanh((1 - s / p) 100 / m) m / 100, every mode is out[b,c,t] = u[b,c,t] F[b,c,t],
 * then out -= mask out.  The factor entries run one thread per (b, c) over the time window with every scalar in
 * fp64 and write one fp32 value per plane; the apply entries are the fp32 element-wise passes.  All four refuse null
 * pointers, non-positive extents, more than 65535 planes, an unknown mode and an m that is not finite and positive. */
#define NPS_VOLUME_BLOCK 0
#define NPS_VOLUME_INDIVIDUAL 1
/* F[B*c*tw].  block: Sm = mean_t s_t, F_t = p r(Sm, p) / Sm for every t.
 * individual: p_0 = p, r_i = r(s_i, p_i), F_i = r_i p_i / s_i, p_{i+1} = r_i p_i. */
int nps_volume_factors(const double* new_tot, const double* prev_tot, int mode, double max_pct_dif, float* F, int B,
                       int num_c, int tw, void* stream);
/* c[B*c*tw], c_t = sum_t' D_t' dF_t'/ds_t with D[B*c*tw] = sum_hw g (1 - mask) u (nps_plane_dot).
 * block: th = tanh((1 - Sm / p) 100 / m), c_t = (sum_t' D_t') ((1 - th^2) / Sm - p r / Sm^2) / tw for every t.
 * individual: the forward recurrence is recomputed (ws[B*c*tw] doubles receive p_i; ws may be NULL for block), then
 * from i = tw - 1 down with lambda = 0: a = D_i / s_i + lambda, c_i = -D_i r_i p_i / s_i^2 + a (1 - th_i^2),
 * lambda = a (r_i - (1 - th_i^2) s_i / p_i). */
int nps_volume_factors_bwd(const double* new_tot, const double* prev_tot, const double* D, int mode,
                           double max_pct_dif, double* ws, float* c, int B, int num_c, int tw, void* stream);
/* in place: u[plane] *= F[plane], then u -= mask[b][mask_ch] u (mask (B, mask_S, H, W) or NULL) */
int nps_volume_apply(float* u, const float* F, const float* mask, int mask_S, int mask_ch, int B, int num_c, int tw,
                     int H, int W, void* stream);
/* gu[plane] = g (1 - mask[b][mask_ch]) F[plane] + c[plane] */
int nps_volume_apply_bwd(const float* g, const float* F, const float* c, const float* mask, int mask_S, int mask_ch,
                         float* gu, int B, int num_c, int tw, int H, int W, void* stream);

/* ---- grid decoders: the per-pixel Conv1d chain + add_delta + tanh + mask (csrc/decode_chain.hip) ----
 * One entry for dec_grid.TimeConvLinear (one stage), TimeConv and TimeConvDense with dec_delta_mode 'all' / 'none'
 * (two stages), and LinearConv's epilogue / add_delta itself (no stage); dec_grid.py:8-31, :34-195.
 * TimeConvDense with 'per_step' and GELU stays on nps_timeconv_decode.
 *
 * Input: a pixel's signal x[ci][l], ci < C0, l < L0, at x[b * x_bs + pix * x_ps + (ci * L0 + l) * x_cs] (element
 * strides): the planar [B][C0*L0][N] is (C0*L0*N, 1, N), channels-last [B][N][C0*L0] is (N*C0*L0, C0*L0, 1).
 * N is the flat pixel count of a 1-D, 2-D or 3-D grid.
 * Stage 1 (nstage >= 1): Conv1d(C0 -> C1, k1, stride s1 >= 1), w1 [C1][C0][k1], b1 [C1]; L1 = (L0 - k1) / s1 + 1; then
 * `act` (NPS_DECODE_ACT_*; Swish is z * sigmoid(beta z)).  Stage 2 (nstage == 2): Conv1d(C1 -> C2, k2, stride 1),
 * w2 [C2][C1][k2], b2 [C2].  The last stage must yield exactly num_c channels x tw positions (nstage == 0:
 * C0 * L0 == num_c * tw); anything else is refused with the sizes in nps_last_error().
 * Epilogue on the chain's output d[c][t]: delta_mode NPS_DECODE_PER_STEP u_last + dtcum[t] * d (dtcum: tw floats, the
 * fp32 cumsum of dt), NPS_DECODE_ALL u_last + dt * d, NPS_DECODE_NONE d; u_last = u[b][c][tw - 1][pix] of the model
 * input u (B, num_c, tw, N) (dec_delta_dt=False is dt = 1 on the caller's side); then tanh when act_tanh; then
 * v - m * v with m = mask[b][mask_ch][pix] of mask (B, mask_S, N), or no mask when NULL.  out: (B, num_c, tw, N).
 * LDS: the kernels keep 64, 32, 16 or 8 pixels' arrays per work-group, the most that fit 160 KiB; a chain whose 8
 * pixels do not fit is refused. */
enum { NPS_DECODE_ACT_NONE = 0, NPS_DECODE_ACT_GELU = 1, NPS_DECODE_ACT_SWISH = 2 };
enum { NPS_DECODE_PER_STEP = 0, NPS_DECODE_ALL = 1, NPS_DECODE_NONE = 2 };
typedef struct {
    const float* x;
    long x_bs, x_ps, x_cs;
    int B, N;
    int nstage;
    int C0, L0;
    int C1, k1, s1;
    int act;
    float beta;
    int C2, k2;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* u;
    int num_c, tw;
    int delta_mode;
    float dt;
    const float* dtcum;
    int act_tanh;
    const float* mask;
    int mask_S, mask_ch;
    float* out;
} nps_decode_t;
int nps_decode_fwd(const nps_decode_t* d, void* stream);
/* Backward given gout = dL/d(out) (B, num_c, tw, N): gx in x's strided layout (d->out is not read), gw1 / gb1 / gw2 /
 * gb2 shaped like the parameters; u gets no gradient.  A NULL pointer skips that gradient.  Parameter gradients need
 * ws, nps_decode_bwd_ws_floats(d) floats: at most 1024 work-groups walk the pixel groups, each sums its
 * (parameter, group) terms (an fp64 wave reduction over a group's pixels) into its own row of ws, and a second kernel
 * adds the rows in a fixed order.  There are no atomics: two runs on the same inputs give identical bits. */
size_t nps_decode_bwd_ws_floats(const nps_decode_t* d);
int nps_decode_bwd(const nps_decode_t* d, const float* gout, float* gx, float* gw1, float* gb1, float* gw2,
                   float* gb2, float* ws, void* stream);

/* ---- 3-D U-Net of the 3-D U-FNO (BASELINE config C5: U-FNO 3D over a time-bundled D x H x W volume) ----
 * The reference builds the 3-D U-Net's ResidualBlock / Down / Middle / Downsample from nn.Conv3d and
 * nn.GroupNorm (proc_unet_modern.py:199-455 with num_spatial_dims=3) but has no 3-D Upsample
 * (models/common.py:103-120 raises); this build defines it per axis as the 2-D rule: circular pad 1,
 * then ConvTranspose3d(k=4, s=2, p=0) (DESIGN.md "3-D U-FNO").  Activations are NDHWC; storage and MFMA
 * arithmetic are bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulate) or exact fp32 (v_mfma_f32_32x32x2_f32). */
typedef struct {
    const void* ptr;            /* [B][D][H][W][C] NDHWC, element type per nps_conv3d_t.bf16 */
    int C, D, H, W;
    int off_d, off_h, off_w;    /* placement in the core frame (crop_Nd: < 0 crops, > 0 zero-pads) */
} nps_src3_t;

typedef struct {
    int nsrc;
    nps_src3_t src[NPS_MAX_SRC];
    int B, Dc, Hc, Wc, Cin;     /* core frame (the virtual concatenation); Cin = sum of src[i].C */
    /* frame extension, per side of every spatial axis: circular by `circ` (circular_pad), then `zpad`
     * zeros; the conv is valid over the extended frame */
    int circ, zpad;
    /* prologue on core-frame values (sources' zeros included): x' = act(GN(x)) */
    const double* gn_stats;     /* [B][G][2] (sum, sum of squares) from nps_gn_stats3d, or NULL */
    const float* gn_gamma;      /* [Cin] */
    const float* gn_beta;
    int gn_groups;
    float gn_eps;
    int pre_act;                /* 0 none, 1 GELU(erf) */
    int K, stride;              /* K^3 taps; K in {1, 2, 3}, stride 1 or 2 (K = 3) */
    int transposed;             /* 1: a k4/s2 ConvTranspose3d as 8 phase convs with K = 2, stride 1 */
    int Dout, Hout, Wout;       /* conv output positions (per phase) */
    const void* wpack;          /* nps_conv3d_pack_weights layout */
    const float* bias;          /* [Cout] or NULL */
    int Cout;
    /* epilogue: destination index per axis = m*out_os + out_off (+ the phase bit when transposed);
     * positions outside [0, out_D) x [0, out_H) x [0, out_W) are skipped (crop) */
    void* out;
    int out_C, out_D, out_H, out_W, out_os, out_off_d, out_off_h, out_off_w;
    int accumulate;             /* out += result (crop_Nd(h) + shortcut, proc_unet_modern.py:250) */
    const void* addend;         /* indexed like out, or NULL (proc_ufno.py:118 h_fno + h_unet) */
    int act;                    /* 0 none, 1 GELU, after bias + addend */
    int bf16;                   /* 1: bf16 storage / bf16 MFMA; 0: fp32 storage / exact fp32 MFMA */
    /* [B][NPS_STATS_SUB][2] fp64 or NULL: the launch ADDS the (sum, sum of squares) of the values it stores
     * (as stored: bf16-rounded for bf16 storage; after addend and act) — with accumulate, of the change (stored
     * minus replaced value), as nps_conv2d_t.out_stats — the GroupNorm(1) moments of its output, carried to the
     * next frame instead of an nps_gn_stats3d pass. */
    double* out_stats;
} nps_conv3d_t;

/* Conv3d weight (Cout, Cin, K, K, K) or, transposed != 0, ConvTranspose3d weight (Cin, Cout, 4, 4, 4) ->
 * the kernel's packing ([phase][64-channel Cout tile][kd][16-channel Cin chunk][kh][kw][64][16], zero
 * padded), fp32 or bf16 elements.  nps_conv3d_packed_bytes gives the buffer size. */
size_t nps_conv3d_packed_bytes(int Cout, int Cin, int K, int transposed, int bf16);
int nps_conv3d_pack_weights(const float* w, void* wpack, int Cout, int Cin, int K, int transposed, int bf16,
                            void* stream);
int nps_conv3d_fwd(const nps_conv3d_t* a, void* stream);
/* Test hooks (host code only).  nps_conv3d_route writes into buf[n] the name of the kernel instantiation
 * nps_conv3d_fwd would launch for *a — "conv3d_kernel<bf16|f32,K,S,TH,SIMPLE|GENERAL,REG|REG_O4|DMA|DMA_O4>" or
 * "conv3d_1x1_kernel<NCB,NCH,PRO|PLAIN>" — through the same argument checks and dispatch, without a launch or
 * any other HIP call (the pointers in *a are only compared with NULL).  nps_conv3d_1x1_set_grid: run the bf16
 * 1x1x1 kernel on `wgs` work-groups per sample (> 0; 0 = one resident round, the default), so every wave walks
 * several tiles of a small volume. */
int nps_conv3d_route(const nps_conv3d_t* a, char* buf, int n);
int nps_conv3d_1x1_set_grid(long wgs);
/* act(GN(frame)) of a's core frame (sources, GroupNorm prologue, pre_act) materialised once as
 * out[B][Dc][Hc][Wc][Cpad] (channels >= Cin zero, Cpad % 8 == 0, Cpad <= 1024): the conv that follows reads one aligned
 * source without a prologue (the fused prologue recomputes each element for every depth tap and halo). */
int nps_frame_pack3d(const nps_conv3d_t* a, void* out, int Cpad, void* stream);
/* GroupNorm moments of a core frame (a's sources and B, Dc, Hc, Wc, Cin, bf16): ADDS per (b, group) the
 * fp64 (sum, sum of squares) of the frame's values (uncovered positions count as 0) to stats[B][G][2] */
int nps_gn_stats3d(const nps_conv3d_t* a, int G, double* stats, void* stream);

/* ---- 3-D conv backward (fp32 training of Conv3d and the 3-D Upsample) ----
 * Input gradients are nps_conv3d_fwd launches on dy with weights derived from the parameter (nps_hip/autograd.py
 * Conv3dFn / ConvTranspose3dFn); the entries below provide the rest.
 *
 * Weight gradient on exact fp32 MFMA (v_mfma_f32_32x32x2_f32, fp32 accumulate):
 *   g[m][n][(kd*K + kh)*K + kw] += sum_{b,pd,ph,pw} a[b][pd][ph][pw][m] * Xext[b][pd*S + kd][ph*S + kh][pw*S + kw][n]
 * Xext = x extended per side of every axis by `circ` voxels circularly, then `zpad` zeros (nps_conv3d_t.circ /
 * .zpad); a's extent must be the valid K^3 / stride-S conv's output over Xext.  With a = dy and x = the conv's
 * input, g is nn.Conv3d.weight.grad [Cout][Cin][K][K][K]; with K = 4, S = 2, a = the (circularly padded) input of a
 * k4/s2 transposed conv and x = dy, g is nn.ConvTranspose3d.weight.grad [Cin][Cout][4][4][4]. */
typedef struct {
    const float* a; int B, Da, Ha, Wa, M;     /* [B][Da][Ha][Wa][M] */
    const float* x; int Dx, Hx, Wx, N;        /* [B][Dx][Hx][Wx][N] */
    int K, stride, circ, zpad;                /* K in {1,2,3,4}, stride in {1,2} */
    float* g;                                 /* [M][N][K*K*K], accumulated with += */
} nps_wgrad3d_t;
int nps_conv3d_wgrad(const nps_wgrad3d_t* p, void* stream);
/* Host only: the number of work-groups that share one (m tile, n tile, tap group)'s voxel reduction in that launch
 * (each adds its partial into g atomically), or < 0 where nps_conv3d_wgrad would refuse p. */
int nps_conv3d_wgrad_splits(const nps_wgrad3d_t* p);
/* out[B][Dq][Hq][Wq][8 C], channel ((rd*2 + rh)*2 + rw)*C + c = x[b][2 dq + rd][2 hq + rh][2 wq + rw][c] (0 outside
 * x [B][D][H][W][C]): a K = 4 / stride-2 conv of x is a K = 2 / stride-1 conv of out */
int nps_space_to_depth3d(const float* x, float* out, int B, int D, int H, int W, int C, int Dq, int Hq, int Wq,
                         void* stream);
/* circular pad by `pad` voxels per side of every axis of x [B][D][H][W][C] (out [B][D+2p][H+2p][W+2p][C]), and its
 * adjoint: gx = the wrap-sum of gp [B][D+2p][H+2p][W+2p][C] */
int nps_circular_pad3d(const float* x, float* out, int B, int D, int H, int W, int C, int pad, void* stream);
int nps_circular_fold3d(const float* gp, float* gx, int B, int D, int H, int W, int C, int pad, void* stream);

/* ---- 3-D frame of the differentiable U-Net walk (fp32 only: a->bf16 != 0 is refused) ----
 * The frame is described by nps_conv3d_t's sources and offsets, B, Dc, Hc, Wc, Cin, the GroupNorm fields and pre_act;
 * its conv fields are ignored.
 *
 * nps_frame3d_fwd: out[B][Dc][Hc][Wc][Cin] = act(GN(frame)) with exactly Cin channels (no channel padding; the erf
 * GELU whose derivative the backward uses).  Without prologue and activation this is crop_Nd in 3-D. */
int nps_frame3d_fwd(const nps_conv3d_t* a, float* out, void* stream);
/* Its backward, the 3-D form of nps_frame_pack_bwd2: gy = dL/d(frame) [B][Dc][Hc][Wc][Cin]; gy_plain (or NULL) = the
 * gradient of the un-normalised concatenation of the same sources, shaped like gy, added into dsrc in the same pass.
 * dsrc[i] (shape of source i; a NULL entry is skipped) receives source i's gradient, exactly 0 at its voxels
 * outside the frame; dgamma / dbeta [Cin] are written when the frame has a GroupNorm; work = [B][2][Cin] fp64 that
 * holds zeros on entry.  The group size N counts the whole frame (uncovered positions are zeros that take part in the
 * statistics, as in nps_gn_stats3d). */
int nps_frame3d_bwd(const nps_conv3d_t* a, const float* gy, const float* gy_plain, float* const* dsrc, float* dgamma,
                    float* dbeta, double* work, void* stream);
/* out = base + crop_Nd(src) placed at (off_d, off_h, off_w) in one pass (out, base: [B][Do][Ho][Wo][C]; src:
 * [B][Ds][Hs][Ws][C]); offsets of either sign per axis (> 0 zero-pads, < 0 crops); any C. */
int nps_add_at_copy3d(float* out, const float* base, const float* src, int B, int Do, int Ho, int Wo, int Ds, int Hs,
                      int Ws, int C, int off_d, int off_h, int off_w, void* stream);
/* Test hook (host code only, no HIP call): 1 and the frame coordinates (fd, fh, fw) when voxel (d, h, w) of source
 * si lies inside a's core frame, 0 when it lies outside, < 0 on bad arguments or if the two directions of the
 * kernels' voxel decode disagree.  It runs the same __host__ __device__ index functions as the three entries above. */
int nps_frame3d_locate(const nps_conv3d_t* a, int si, int d, int h, int w, int* fd, int* fh, int* fw);

/* ---- U-Net self-attention (proc_unet_modern.py:292-317), never materialising the N x N scores ----
 * Layouts, exactly as the qkv projection writes them (no q / k / v split copies):
 *   qkv, dqkv [B][N][heads][3*dk]  (per head [q | k | v], dk floats each)
 *   out, dout [B][N][heads*dk]
 *   lse       [B][heads][N]
 * The reference's softmax runs over the QUERY index i for each key j (softmax(dim=1)):
 *   P[i][j] = exp(scale q_i.k_j - lse[j]),  lse[j] = log sum_i exp(scale q_i.k_j),  out_i = sum_j P[i][j] v_j.
 * nps_attn_colstats computes lse (per key tile, an online max / sum over query tiles); nps_attn_fwd then needs
 * no running rescale.  nps_attn_bwd writes every element of dqkv (dV_j = sum_i P dO_i, delta_j = dV_j.v_j,
 * dS = P (dO_i.v_j - delta_j), dK_j = scale sum_i dS q_i, dQ_i = scale sum_j dS k_j; P recomputed from lse) and
 * uses ws[nps_attn_bwd_ws_floats(...)] floats of scratch (delta).  Exact-fp32 MFMA, fp32 expf.
 * dk % 4 == 0, 4 <= dk <= 256; heads, B >= 1 (<= 65535); N >= 1; 16-byte aligned tensors.  Anything else
 * returns < 0 with nps_last_error set. */
int nps_attn_colstats(const float* qkv, float* lse, int B, int N, int heads, int dk, float scale, void* stream);
int nps_attn_fwd(const float* qkv, const float* lse, float* out, int B, int N, int heads, int dk, float scale,
                 void* stream);
size_t nps_attn_bwd_ws_floats(int B, int N, int heads, int dk);
int nps_attn_bwd(const float* qkv, const float* lse, const float* dout, float* dqkv, float* ws, int B, int N,
                 int heads, int dk, float scale, void* stream);

/* ---- 1-D U-Net convs (fp32, exact-fp32 MFMA v_mfma_f32_32x32x2_f32): k-tap Conv1d along L ----
 * Activations are channels-last [B][L][C] fp32, contiguous.  The input is a virtual frame of Lc positions and Cin
 * channels: the channel concatenation of up to NPS_MAX_SRC sources, source i placed at frame position off (crop_Nd:
 * off > 0 zero-pads, off < 0 crops; a source shorter than the frame reads as zero outside itself).  Everything
 * outside [0, Lc) of the same sample is zero.
 *   y[b][l][co] = bias[co] + sum_{t < K, ci} W[co][ci][t] * frame[b][l*stride + t - pad_l][ci],  l < Lout,
 *   Lout = (Lc + pad_l + pad_r - K) / stride + 1 (checked),
 *   v = act(y + addend[b][ol][co]),  ol = l*out_os + out_off; rows with ol outside [0, out_L) are dropped,
 *   out[b][ol][co] = v, or += v with accumulate.  addend (or NULL) is laid out like out.
 * K in 1..4, stride in {1, 2}, out_os in {1, 2}; Cin, Cout >= 1 (no multiple required: the packed weight and the
 * staged tiles are zero-padded).  A k4/s2 transposed conv is its two 2-tap phases with out_os = 2; a conv's input
 * gradient is this entry over dy with a derived weight (nps_hip/autograd.py Conv1dFn / ConvTranspose1dFn). */
typedef struct {
    const float* ptr; int C, L, off;
} nps_src1_t;
typedef struct {
    int nsrc;
    nps_src1_t src[NPS_MAX_SRC];
    int B, Lc, Cin;                           /* Cin = sum of the sources' C */
    int K, stride, pad_l, pad_r, Lout;
    const float* wpack;                       /* nps_conv1d_pack_weights of W [Cout][Cin][K] */
    const float* bias;                        /* [Cout] or NULL */
    int Cout;
    float* out; int out_C, out_L, out_os, out_off;   /* out [B][out_L][out_C], out_C >= Cout */
    int accumulate;
    const float* addend;
    int act;                                  /* 0 none, 1 GELU (erf) */
} nps_conv1d_t;
/* floats of the packing [K][Cin padded to 16][Cout padded to 64] */
size_t nps_conv1d_packed_floats(int Cout, int Cin, int K);
int nps_conv1d_pack_weights(const float* w, float* wpack, int Cout, int Cin, int K, void* stream);
int nps_conv1d_fwd(const nps_conv1d_t* p, void* stream);
/* Weight gradient: g[m][n][t] = sum_{b,l} a[b][l][m] * xz[b][l*stride + t - pad_l][n] (xz = x, zero outside [0, Lx));
 * La = (Lx + pad_l + pad_r - K) / stride + 1 (checked).  With a = dy, x = the conv's input: nn.Conv1d.weight.grad
 * [Cout][Cin][K]; with K = 4, stride = 2, a = a k4/s2 transposed conv's input and x = dy: nn.ConvTranspose1d
 * .weight.grad [Cin][Cout][4].  The (b, l) reduction is split over work-groups by a schedule fixed by the shape;
 * every split stores its partial to ws [nps_conv1d_wgrad_ws_floats(p)] and a second launch sums them in split order
 * and stores g (no atomics: two runs give identical bits). */
typedef struct {
    const float* a; int B, La, M;             /* [B][La][M] */
    const float* x; int Lx, N;                /* [B][Lx][N] */
    int K, stride, pad_l, pad_r;
    float* g;                                 /* [M][N][K], stored */
    float* ws;
} nps_wgrad1d_t;
size_t nps_conv1d_wgrad_ws_floats(const nps_wgrad1d_t* p);   /* 0 where nps_conv1d_wgrad would refuse p */
int nps_conv1d_wgrad(const nps_wgrad1d_t* p, void* stream);

const char* nps_last_error(void);
const char* nps_version(void);

/* ---- on-disk data path: device-resident windowing (common/data_creator.py:48-78, create_data) ----
 * out[b][c][t][hw] = u[b][c][steps[b] + offset + t][hw], t < tw; u (B, C, T, H*W) and out (B, C, tw, H*W)
 * contiguous fp32 device arrays, steps[B] int32 on the device (offset = -tw: model inputs, 0: labels;
 * the caller checks steps[b] + offset >= 0 and steps[b] + offset + tw <= T, as the reference asserts). */
int nps_gather_windows(const float* u, const int* steps, float* out, int B, int C, int T, long HW, int tw, int offset,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NPS_H */
