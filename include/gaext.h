/* libgaext -- C ABI of the MI355X (gfx950) kernels for the GA-ConvNeXt / GA / MAP training hot path.
 *
 * The reference (Lab-LVM/imagenet-models) has NO native layer: its hot path is the list of ATen ops that
 * GA/ga_convnext.py, GA/train.py execute.  Each entry point below replaces the ATen
 * op(s) named in its comment (file:line = /root/reference/...).  Conventions:
 *
 *  - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (the library never
 *    allocates, frees or synchronises: the two entry points that reduce per-workgroup partial results take a
 *    caller-owned workspace sized by their ga_*_workspace() query); every call only ENQUEUES work on the
 *    hipStream_t passed last.
 *  - activations are NHWC ("channels last"), i.e. 2-D row-major [rows = B*H*W, C]; `dtype` selects the
 *    element type of activations and of the prepared ("effective") weight copies: GA_F32 = the parity math
 *    mode, GA_BF16 = the throughput mode (fp32 accumulation, fp32 statistics, fp32 master weights/gradients).
 *  - return 0 on success; <0 on error (GA_ERR_*), message retrievable with ga_last_error (thread-local).
 *  - 16-byte alignment of every activation / weight-copy pointer and leading dimensions that are multiples of
 *    8 elements are required (GA_ERR_BAD_ARG otherwise).
 */
#ifndef GAEXT_H
#define GAEXT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ga_stream_t; /* hipStream_t */

enum { GA_F32 = 0, GA_BF16 = 1 };
enum { GA_OK = 0, GA_ERR_BAD_ARG = -1, GA_ERR_UNSUPPORTED = -2, GA_ERR_HIP = -3 };

/* activation codes */
enum { GA_ACT_NONE = 0, GA_ACT_GELU = 1, GA_ACT_RELU = 2 };

/* A-operand gather kinds (implicit im2col): how row m / column k of the GEMM's A matrix map to memory */
enum {
    GA_A_PLAIN = 0,      /* A[m*lda + k]                                                              */
    GA_A_PATCH2 = 1,     /* NHWC [B,H,W,C] -> rows (b,oy,ox) of the 2x2/s2 patches, k = (ky,kx,c)    (ga_convnext.py:127) */
    GA_A_STEM4_NCHW = 2, /* fp32 NCHW [B,3,H,W] -> rows (b,oy,ox) of the 4x4/s4 patches, k=(c,ky,kx) (ga_convnext.py:357) */
    GA_A_CONV3 = 3,      /* NHWC [B,H,W,C], 3x3 pad 1 stride 1, k = (ky,kx,c)                         (ga_convnext.py:273) */
    GA_A_CONV3S2 = 4,    /* NHWC [B,H,W,C], 3x3 pad 1 stride 2 -> rows (b,oy,ox) of the [(H+1)/2, (W+1)/2] output,
                            k = (ky,kx,c): the deep stem and Merge_Block convs        (ga_cswin.py:464,474,256) */
    GA_A_NEIGH2 = 5      /* NHWC [B,H,W,C], rows (b,y,x), k = (ay,ax,c) reads pixel (y+ay, x+ax), ay,ax in {0,1}, zero
                            beyond the map: with ga_conv3s2_dgrad_prep's operand and GA_C_UNPATCH2 it is the
                            data-gradient (transposed convolution) of GA_A_CONV3S2 */
};
/* C-output kinds */
enum {
    GA_C_PLAIN = 0,
    GA_C_UNPATCH2 = 1 /* rows (b,oy,ox), cols (ky,kx,c) scattered back to NHWC [B,H,W,C] (dgrad of the 2x2/s2 conv) */
};

int ga_version(void);
/* copies the calling thread's last error message (NUL-terminated) into buf; returns its length */
int ga_last_error(char* buf, size_t n);
/* number of compute units / LDS per CU etc. of the current device (used for grid sizing); 0 on success */
int ga_device_info(int* num_cu, int* lds_bytes, int* wave_size);

/* Tuning knobs (kernel-form selection; no reference counterpart -- the reference delegates kernel choice to cuDNN / cuBLAS
 * heuristics behind torch.backends.cudnn.benchmark, GA/train.py:400).  Each knob NAME takes its value from the environment
 * variable GAEXT_<NAME> once, when the dispatch code first asks for it, or from ga_set_knob(); no launch ever reads the
 * environment.  ga_unset_knob() returns a knob to its built-in default.  ga_config_string() writes "libgaext <version> gfx950"
 * followed by every knob that is NOT at its default as " NAME=value(env|api)" (NUL-terminated, truncated to n) and returns
 * the untruncated length -- a bench / parity record shows what actually ran.  Result-changing debug switches do not exist in a
 * release build (they need -DGAEXT_DEBUG, which ga_config_string reports as DEBUG-BUILD). */
int ga_set_knob(const char* name, int value);
int ga_unset_knob(const char* name);
int ga_config_string(char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------------------
 * ga_gemm:  C[z][m][n] = epilogue( alpha * sum_k A[z][m][k] * B[z][n][k] )          (both operands K-contiguous)
 * replaces: nn.Linear / 1x1, 2x2-s2, 4x4-s4 and 3x3 nn.Conv2d forward AND their data-gradients
 *           (ga_convnext.py:94,127,163-167,202-205,259-283,357,407,418,422) -- dgrad uses the transposed
 *           weight copy made by ga_weight_prep, so it is the same NT product.
 * epilogue order: v = alpha*acc; v += bias[n]; (C2 store); v = act(v); v *= dact(H[m][n]) (GELU'); v *= rowscale[m / rows_per_scale];
 *                 v += R[m][n]; if (relu_after) v = max(v,0); colsum[n] += v; colsumsq[n] += v*v; store.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    int batch;             /* grid z (>=1) */
    int dtype;             /* GA_F32 / GA_BF16: type of A, B, R, H (and of C unless c_f32) */
    /* A */
    const void* A;
    int64_t lda, strideA;
    int a_batch_mod;       /* A batch index = z % a_batch_mod (0: = z) */
    int a_kind;            /* GA_A_* */
    int a_H, a_W, a_C;     /* input dims for the gather kinds */
    int a_act;             /* GA_ACT_*: applied to A elements while staging (GELU of a stored pre-activation) */
    /* B (weights, [N][K] K-contiguous) */
    const void* B;
    int64_t ldb, strideB;
    /* C */
    void* C;
    int64_t ldc, strideC;
    int c_kind;            /* GA_C_* */
    int c_H, c_W, c_C;     /* NHWC dims of the scatter target (GA_C_UNPATCH2) */
    int c_f32;             /* 1: C is fp32 regardless of dtype */
    void* C2;              /* optional second output (dtype, layout of C): see c2_mode */
    int c2_mode;           /* 1: the pre-activation value (alpha*acc + bias); 2: act'(pre-activation) (GELU') -- lets the
                              forward fc1 store gelu(h) AND gelu'(h) so that backward never re-evaluates erf */
    /* epilogue */
    float alpha;
    const float* bias;     /* [N] or NULL */
    int64_t strideBias;
    int act;               /* GA_ACT_* */
    const void* H;         /* GELU-backward: multiply by gelu'(H[m][n]) (dtype), or NULL */
    int64_t ldh, strideH;
    int h_is_deriv;        /* 1: H already holds the derivative (stored by c2_mode 2): multiply by H[m][n] itself */
    const float* rowscale; /* per-sample scale (DropPath mask / keep) or NULL */
    int rows_per_scale;
    const void* R;         /* residual (dtype) or NULL */
    int64_t ldr, strideR;
    int relu_after;
    float* colsum;         /* [N] fp32 atomics, or NULL  (BatchNorm batch statistics / bias gradients) */
    float* colsumsq;       /* [N] fp32 atomics, or NULL */
    int64_t strideCol;
} ga_gemm_desc;
int ga_gemm(const ga_gemm_desc* d, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * ga_wgrad:  dW[z][n][k] (+)= alpha * sum_m Y[z][m][n] * X[z][m][k]              (reduction over the ROW index)
 * replaces: the weight-gradient of every Linear/Conv2d above (ATen convolution_backward / mm in autograd) and,
 *           with Y == X, the Gram product X.X^T of GA_ConvNeXt.get_gram (ga_convnext.py:459-460).
 * The M range is split over `split_m` workgroups that combine with fp32 atomics (split_m == 1: plain store when
 * accumulate == 0).  dbias[n] += sum_m Y[m][n] when dbias != NULL.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    int batch;
    int dtype;
    const void* Y;
    int64_t ldy, strideY;
    const void* X;
    int64_t ldx, strideX;
    int x_batch_mod;       /* X batch index = z % x_batch_mod (0: = z) */
    int x_kind;            /* GA_A_* gather of X rows */
    int x_H, x_W, x_C;
    int x_act;             /* GA_ACT_GELU: X := gelu(X) while staging */
    float* dW;             /* fp32 [N][ldw] */
    int64_t ldw, strideW;
    float* dbias;          /* fp32 [N] or NULL */
    int64_t strideDbias;
    float alpha;
    int split_m;           /* >=1 */
    int accumulate;        /* 1: add into dW (atomics); 0 with split_m==1: overwrite */
    void* workspace;       /* caller-owned device scratch of ga_wgrad_workspace(d) bytes (16-byte aligned), or NULL: the wide */
    int64_t ws_bytes;      /* form then combines its row splits with fp32 atomics instead of partial tiles + a reduce launch */
} ga_wgrad_desc;
int ga_wgrad(const ga_wgrad_desc* d, ga_stream_t stream);
/* bytes of scratch ga_wgrad would like for this descriptor (0: none).  Concurrent calls (different streams) need distinct
 * workspaces; calls on one stream may share one. */
size_t ga_wgrad_workspace(const ga_wgrad_desc* d);

/* Which kernel form ga_gemm / ga_wgrad launches for a descriptor under the current knob table.  Validates exactly as the launch
 * does (same return code, same ga_last_error message) and, on GA_OK, writes the form's stable name into buf (NUL-terminated,
 * truncated to n).  Touches no device memory and launches nothing: it also works on a machine without a GPU, where the number
 * of compute units is taken as 256.  The forms in the order they are tried, ":epilogue" = plain | fc1 | fc2 | dg2 | generic:
 *   ga_gemm:  conv3_direct, conv0_direct          direct convolutions (64 -> 64 channels 3x3; 3 (8) -> 64 stride 2)
 *             r3g:plain                           3-slot ring, 3x3/s2 and 2x2-neighbourhood gathers
 *             r3:<epi>                            3-slot ring, 256 x 128 tiles (also GA_A_PATCH2 / GA_C_UNPATCH2 as r3:plain)
 *             dma256x128:<epi> dma256x96:<epi>    256-row LDS-DMA tiles
 *             pp:<epi>                            8-wave ping-pong, 256 x 256
 *             t256:<epi>                          256 x 256 LDS-DMA
 *             dma128:<epi>                        128 x 128 LDS-DMA
 *             big:<epi>                           256 x 128 register-staged (fc2, dg2)
 *             staged128|96|64:<epi>[+pre][+gather][+f32]   register-staged 128-row tiles: +pre prefetches the epilogue operand,
 *                                                 +gather reads a gathered A, +f32 is the fp32 instantiation
 *   ga_wgrad: conv3_wgrad_direct:wgs<G>, conv3s2_wgrad_direct:.., conv0_wgrad_direct:.., stem4_wgrad_direct:..   G workgroups with
 *                                                 64*576 (conv0: 64*72, stem4: N*49) floats of workspace each; need d->workspace
 *             tn2:split<S>:partials|atomics       wide 256 x 256 form with S row splits (partials: batch*S*N*K floats of
 *                                                 workspace); tn2p: on a GA_A_PATCH2 operand
 *             tn                                  128 x 128 form, split_m row splits */
int ga_gemm_form(const ga_gemm_desc* d, char* buf, size_t n);
int ga_wgrad_form(const ga_wgrad_desc* d, char* buf, size_t n);

/* Few-row forms (gemm_fewrows.hip): the same products for launches with few rows (M <= 512: the heads' one row per image) that
 * ga_gemm / ga_wgrad would run on a handful of 128-row tiles -- fewer tiles x batch than half the compute units.  Same descriptors,
 * same validation, same results up to the fp32 summation order; bf16, plain layouts only.
 *   ga_gemm_fewrows:  32 x 32 output tile per workgroup, the four waves split K, no LDS staging of the operands.  Takes bias, alpha,
 *                     c_f32, rowscale, R, colsum / colsumsq, the fc1 epilogue (GELU, C2 with c2_mode 2) and H with h_is_deriv.
 *   ga_wgrad_fewrows: 64 x 64 output tile per workgroup with the whole reduction inside: no split_m, no atomics between workgroups,
 *                     so dW and dbias come out bit-identical from run to run.
 * A descriptor they do not take -- or any descriptor when the knob FEWROWS is 0 -- is forwarded to ga_gemm / ga_wgrad unchanged.
 * The _form queries work like ga_gemm_form and name what the entry point would do itself: fewrows32x32:<epilogue>,
 * fewrows_tn64x64, or "none" (forwarded). */
int ga_gemm_fewrows(const ga_gemm_desc* d, ga_stream_t stream);
int ga_wgrad_fewrows(const ga_wgrad_desc* d, ga_stream_t stream);
int ga_gemm_fewrows_form(const ga_gemm_desc* d, char* buf, size_t n);
int ga_wgrad_fewrows_form(const ga_wgrad_desc* d, char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------------------
 * Weight preparation: fp32 master conv/linear weight [G*Co][Ci][KH][KW]  ->  "effective" copies in `dtype`
 *   out [G][Co][ldo]  with k = (ky,kx,ci)   : out = rs[n] * w * cs[ci]          (B operand of the forward GEMM)
 *   outT[G][KH*KW*Ci][ldt] (co contiguous)  : transposed copy                   (B operand of the dgrad GEMM);
 *        flip=1: outT is [G][Ci][ldt >= KH*KW*Co] with column ((KH-1-ky)*KW + KW-1-kx)*Co + co
 *        (dgrad of a stride-1 'same' conv as a GA_A_CONV3 product over dY).
 *   stem=1: k = (ci,ky,kx) (the NCHW patch order of GA_A_STEM4_NCHW).
 * Folds LayerNorm scale (cs) / LayerScale gamma (rs) into the weights (ga_convnext.py:93,95,106,110).
 * Pads [.., ldo) / [.., ldt) with zeros.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* w;
    int G, Co, Ci, KH, KW;
    const float* rs;       /* [G*Co] or NULL (indexed by the SOURCE row) */
    const float* cs;       /* [Ci] or NULL */
    const int* row_perm;   /* [G*Co] or NULL: effective row n is master row row_perm[n] (channel_shuffle, ga_convnext.py:217,557) */
    int dtype;
    void* out;  int64_t ldo;   /* may be NULL */
    void* outT; int64_t ldt;   /* may be NULL */
    int flip;
    int stem;
    int t_cols;            /* columns of every outT row this job writes (incl. zero padding), 0 = ldt: several jobs
                            * may fill column ranges of ONE stacked transposed operand of row stride ldt */
} ga_wprep_desc;
int ga_weight_prep(const ga_wprep_desc* d, ga_stream_t stream);
/* be[n] = rs[m] * (b[m] + sum_c W[m][c] * v[c]), m = row_perm ? row_perm[n] : n   (W fp32 [N][C]; b, rs, v may be NULL) */
int ga_bias_fold(const float* W, const float* b, const float* rs, const float* v, const int* row_perm, float* be, int N,
                 int C, ga_stream_t stream);
/* Inverse of the folding for gradients. G = d(effective weight) fp32 [N][ldg] with k=(ky,kx,ci); gb = d(effective bias),
 * where We = rs[n]*W*cs[ci] and be[n] = rs[n]*(b[n] + sum_c W[n][c]*v[c]):
 *   dW[n][ci][ky][kx] += rs[n]*(G*cs[ci] + gb[n]*v[ci]);  d_cs[ci] += sum rs[n]*G*W;
 *   d_rs[n] += sum_k G*W*cs[ci] + gb[n]*(b[n] + sum_c W*v);  d_v[ci] += sum_n gb[n]*rs[n]*W[n][ci];  db[n] += rs[n]*gb[n].
 * cs / v / d_cs / d_v need KH=KW=1.  Any output may be NULL. */
typedef struct {
    const float* G; int64_t ldg;
    const float* gb;
    const float* W; const float* b;
    const float* rs; const float* cs; const float* v;
    const int* row_perm;   /* rows of G / gb are effective rows; master row = row_perm[n] */
    int N, Ci, KH, KW;
    int stem;
    float* dW; float* db; float* d_rs; float* d_cs; float* d_v;
} ga_wunfold_desc;
int ga_weight_unfold(const ga_wunfold_desc* d, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Depthwise 7x7 (pad 3) convolution, NHWC  (ga_convnext.py:92,100)
 *   w49: fp32 [49][C] (tap-major copy of conv_dw.weight), bias fp32 [C]
 * ------------------------------------------------------------------------------------------------------------ */
int ga_dwconv7_fwd(const void* x, const float* w49, const float* bias, void* y, int B, int H, int W, int C,
                   int dtype, ga_stream_t stream);
/* dx = res + conv7x7(dy, flipped w)   (res may be NULL) */
int ga_dwconv7_bwd_data(const void* dy, const float* w49, const void* res, void* dx, int B, int H, int W, int C,
                        int dtype, ga_stream_t stream);
/* the same with a second output dx2[b,...] = dx[b,...] (as stored) * scale2[b]: the next block's DropPath row scale
 * (x.div(keep) * mask, timm DropPath behind GA/ga_convnext.py:111) applied where dx is produced instead of by a
 * separate pass over it; res is required */
int ga_dwconv7_bwd_data2(const void* dy, const float* w49, const void* res, void* dx, void* dx2, const float* scale2,
                         int B, int H, int W, int C, int dtype, ga_stream_t stream);
/* dw49[49][C] += sum dy * shifted x ; dbias[C] += sum dy   (per-workgroup partial sums in the CALLER-provided workspace of
 * ga_dwconv7_bwd_weight_workspace(...) bytes, then one reduction launch; deterministic for a fixed grid) */
size_t ga_dwconv7_bwd_weight_workspace(int B, int H, int W, int C, int dtype);
int ga_dwconv7_bwd_weight(const void* dy, const void* x, float* dw49, float* dbias, int B, int H, int W, int C,
                          int dtype, void* workspace, size_t ws_bytes, ga_stream_t stream);
/* Which kernel form the entry points above launch for a geometry under the current knob table, in the manner of ga_gemm_form:
 * same validation of the geometry (GA_ERR_BAD_ARG with a message), on GA_OK the form's stable name in buf (NUL-terminated,
 * truncated to n; buf may be NULL), no device memory touched, nothing launched, 256 compute units assumed without a GPU.  The
 * launches run what the same host functions return (csrc/dwconv.hip: dw_select, dww_select), so the name is what runs.
 *   ga_dwconv7_form (forward: has_res = has_y2 = 0; backward-data: has_res = res != NULL; _bwd_data2: both 1), as tried:
 *     rs:R<r>:seg<s>:wpu<w>[+res][+y2]   register-sliding LDS-DMA form (bf16, C % 8 == 0, H % 7 == 0, below 2 GiB; knob DW_RS):
 *                                        r rows per segment (DW_RS_ROWS, else the longest divisor of H that is a multiple of 7
 *                                        with B s w >= 8 waves per CU), s = H / r segments per image, w waves per (image,
 *                                        segment); +res / +y2 name the kernel instantiation
 *     mfma:gx<g>:tiles<t>                Toeplitz form on the matrix cores (bf16, C % 8 == 0, H and W multiples of 14; knob
 *                                        DW_MFMA: 2 always, 1 from 56 x 56 maps with t * ceil(C / 32) >= 16 per CU): g workgroups
 *                                        per 32-channel slice walk t tiles; g is rounded down to a multiple of 8 from 16 (DW_XCD8)
 *     dot2_14x14:gx<g>:tiles<t>          LDS-staged v_dot2 form on 14 x 14 tiles (bf16, C % 8 == 0, H and W multiples of 14)
 *     dot2_7x7:gx<g>:tiles<t>            the same on 7 x 7 tiles (any H, W); g workgroups per 64-channel slice walk t tiles
 *     scalar_14x14+f32|bf16              the scalar template (fp32; bf16 with C % 8 != 0), one workgroup per tile and 32 channels
 *     scalar_7x7+f32|bf16
 *   ga_dwconv7_bwd_weight_form:
 *     rs:R<r>:seg<s>:wpu<w>:nbw<k>       register-sliding form (bf16, C % 8 == 0, H % 7 == 0, below 2 GiB; knob DWW_RS: 1 from
 *                                        28 x 28 maps, 2 everywhere): k w workgroups of 4 waves, k = max(1, 2 CUs / w); the 4 k
 *                                        waves of a lane map walk the B s units; r from DWW_RS_ROWS, else the longest with
 *                                        B s >= 8 k
 *     dot2_14x14:parts<p>  dot2_7x7:parts<p>            p workgroups per 64-channel slice, one partial each
 *     scalar_14x14:parts<p>+f32|bf16  scalar_7x7:..     p partials of p / 2 (14 x 14) or p (7 x 7) workgroups per slice */
int ga_dwconv7_form(int B, int H, int W, int C, int dtype, int has_res, int has_y2, char* buf, size_t n);
int ga_dwconv7_bwd_weight_form(int B, int H, int W, int C, int dtype, char* buf, size_t n);

/* ------------------------------------------------------------------------------------------------------------
 * Depthwise 3x3 (pad 1, stride 1 or 2, no bias) convolution, NHWC [B][H][W][C] -> [B][Ho][Wo][C], Ho = (H - 1) / stride + 1
 * (MobileNetV1's conv_dw, MAP/models/map_mobilenet.py:27-38).  w9: fp32 [C][9], the (C, 1, 3, 3) parameter as it is.
 * C % 8 == 0 and stride in {1, 2} (GA_ERR_UNSUPPORTED otherwise); H, W any size >= 1.
 *   fwd:        colsum / colsumsq (both or neither) accumulate sum_rows y and sum_rows y^2 of the fp32 outputs before rounding
 *               (the batch statistics of the BatchNorm that follows; one atomic per channel per workgroup)
 *   bwd_data:   dx (H x W, overwritten) from dy (Ho x Wo): gather form, no atomics
 *   bwd_weight: dw9[C][9] += sum dy * shifted x; per-workgroup partials in the CALLER-provided workspace of
 *               ga_dwconv3_bwd_weight_workspace(...) bytes, then one reduction launch (deterministic for a fixed shape)
 * ------------------------------------------------------------------------------------------------------------ */
int ga_dwconv3_fwd(const void* x, const float* w9, void* y, int B, int H, int W, int C, int stride, float* colsum,
                   float* colsumsq, int dtype, ga_stream_t stream);
int ga_dwconv3_bwd_data(const void* dy, const float* w9, void* dx, int B, int H, int W, int C, int stride, int dtype,
                        ga_stream_t stream);
size_t ga_dwconv3_bwd_weight_workspace(int B, int H, int W, int C, int stride, int dtype);
int ga_dwconv3_bwd_weight(const void* dy, const void* x, float* dw9, int B, int H, int W, int C, int stride, int dtype,
                          void* workspace, size_t ws_bytes, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * MAP-ResNet50 (MAP/models/map_resnet.py): NHWC, C % 8 == 0 (GA_ERR_UNSUPPORTED otherwise), bf16 / fp32 tensors, fp32 math.
 *   maxpool3s2_fwd:  MaxPool2d(3, 2, 1), any H, W; Ho = (H - 1) / 2 + 1.  PyTorch's rule: the first maximum in row-major window order,
 *                    NaN propagates.  idx (uint8 [B][Ho][Wo][C], window tap 0..8, may be NULL) feeds the backward.
 *   maxpool3s2_bwd:  dx (H x W) = (accumulate ? dx : 0) + the gradients of the outputs that chose each pixel (gather, no atomics)
 *   bn_gelu_fwd:     y = gelu_erf(x * scale[c] + shift[c])
 *   bn_gelu_bwd_reduce: g = dy * gelu'(x * scale + shift), xhat = (x - mean) * rstd; s1[c] = sum g, s2[c] = sum g * xhat (overwritten);
 *                    per-workgroup partials in the caller's workspace of ga_bn_gelu_bwd_workspace(rows, C) bytes, then one ordered
 *                    reduction (deterministic)
 *   bn_gelu_bwd_apply: dx = w * rstd * (g - s1 / n - xhat * s2 / n)   (w NULL -> 1)
 *   se_bn_fwd:       SEUnit with BatchNorm (B <= 1024, C <= 2048, R <= 128; train mode needs B >= 2).  S [B][C] = sum_hw of the raw
 *                    conv output, p = scale3 * S / HW + shift3; hpre = p W1^T (W1 [R][C], no bias); BatchNorm (g1, b1, eps 1e-5)
 *                    over the B rows: batch statistics and the running-stat update (momentum 0.1, unbiased variance) when
 *                    training, the running statistics otherwise (mean / rstd [R] written either way); h = gelu(.);
 *                    gate = sigmoid(h W2^T + b2) (W2 [C][R]).  All fp32.
 *   se_bn_bwd:       from P1 / P2 [B][C] of se_residual_bwd_a: dgate = r * (g3 P2 + b3 P1); writes dz [B][C] and dhpre [B][R]
 *                    (workspaces), ds [B][C] (the gradient of p) and the BatchNorm-3 sums s1 / s2 [C] (overwritten); dW1, dg1, db1,
 *                    dW2, db2 are accumulated (+=) with one owner per element (no atomics)
 *   se_residual_fwd: y = relu(res' + r[b] * gate[b][c] * (x3 * scale3 + shift3)); res' = res * rscale + rshift, or res when both are
 *                    NULL; r = rowscale (DropPath factors, NULL -> 1)
 *   se_residual_bwd_a: dm = dy * (y > 0) (also the residual's gradient); P1 = sum_hw dm, P2 = sum_hw dm * xhat3 per (b, c), one
 *                    workgroup per (sample, channel chunk): no atomics
 *   se_residual_bwd_b: dx3 = g3 * rstd3 * (du - s1 / n - xhat3 * s2 / n), du = dm * gate * r + ds / HW, n = B * HW
 *   subsample2_fwd / _bwd: y[b, oy, ox] = x[b, 2oy, 2ox] (the input of a 1 x 1 / 2 conv, Ho = (H - 1) / 2 + 1); the backward writes
 *                    the zero-filled transpose, or adds into dx at the even pixels when accumulate
 * ------------------------------------------------------------------------------------------------------------ */
int ga_maxpool3s2_fwd(const void* x, void* y, unsigned char* idx, int B, int H, int W, int C, int dtype, ga_stream_t stream);
int ga_maxpool3s2_bwd(const void* dy, const unsigned char* idx, void* dx, int B, int H, int W, int C, int accumulate, int dtype,
                      ga_stream_t stream);
int ga_bn_gelu_fwd(const void* x, const float* scale, const float* shift, void* y, int64_t rows, int C, int dtype, ga_stream_t stream);
size_t ga_bn_gelu_bwd_workspace(int64_t rows, int C);
int ga_bn_gelu_bwd_reduce(const void* dy, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                          float* s1, float* s2, int64_t rows, int C, int dtype, void* workspace, size_t ws_bytes, ga_stream_t stream);
int ga_bn_gelu_bwd_apply(const void* dy, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                         const float* w, const float* s1, const float* s2, int64_t n, void* dx, int64_t rows, int C, int dtype,
                         ga_stream_t stream);
int ga_se_bn_fwd(const float* S, int HW, const float* scale3, const float* shift3, const float* W1, const float* g1, const float* b1,
                 float* rmean, float* rvar, const float* W2, const float* b2, float* hpre, float* mean, float* rstd, float* h, float* gate,
                 int B, int C, int R, int training, ga_stream_t stream);
int ga_se_bn_bwd(const float* P1, const float* P2, const float* rowscale, const float* g3, const float* b3, const float* mean3,
                 const float* rstd3, const float* S, int HW, const float* scale3, const float* shift3, const float* W1, const float* g1,
                 const float* b1, const float* W2, const float* hpre, const float* mean, const float* rstd, const float* h,
                 const float* gate, float* dz, float* dhpre, float* ds, float* s1, float* s2, float* dW1, float* dg1, float* db1,
                 float* dW2, float* db2, int B, int C, int R, ga_stream_t stream);
int ga_se_residual_fwd(const void* x3, const float* scale3, const float* shift3, const float* gate, const float* rowscale, const void* res,
                       const float* rscale, const float* rshift, void* y, int B, int HW, int C, int dtype, ga_stream_t stream);
int ga_se_residual_bwd_a(const void* dy, const void* y, const void* x3, const float* mean3, const float* rstd3, void* dm, float* P1,
                         float* P2, int B, int HW, int C, int dtype, ga_stream_t stream);
int ga_se_residual_bwd_b(const void* dm, const void* x3, const float* mean3, const float* rstd3, const float* g3, const float* gate,
                         const float* rowscale, const float* ds, const float* s1, const float* s2, void* dx3, int B, int HW, int C,
                         int dtype, ga_stream_t stream);
int ga_subsample2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, ga_stream_t stream);
int ga_subsample2_bwd(const void* dy, void* dx, int B, int H, int W, int C, int accumulate, int dtype, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim of [rows][C]  (F.layer_norm / LayerNorm2d, ga_convnext.py:51-67,93,233,237)
 *   fwd: y = (x-mean)*rstd [*w + b];  saves mean/rstd fp32 [rows] (each may be NULL).
 *   bwd: xhat = x_is_normalized ? x : (x-mean)*rstd;
 *        dx = rstd * (g*w - mean_c(g*w) - xhat*mean_c(g*w*xhat)) (+ dres);  dw[c] += sum g*xhat; db[c] += sum g
 *   C > 0, a multiple of 8 (bf16) / 4 (fp32), at most 4096 / 2048; w and b both or neither; dw and db both or neither, and with
 *   them C up to the 64 KB of LDS their reduce takes (bf16: C <= 2048); x / y / g / dres / dx / dx2 16-byte aligned.
 *   GA_ERR_BAD_ARG otherwise, nothing is launched.
 * ------------------------------------------------------------------------------------------------------------ */
int ga_layernorm_fwd(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd, int64_t rows,
                     int C, float eps, int dtype, ga_stream_t stream);
int ga_layernorm_bwd(const void* g, const void* x, const float* mean, const float* rstd, const float* w,
                     const void* dres, void* dx, float* dw, float* db, int64_t rows, int C, int x_is_normalized,
                     int dtype, ga_stream_t stream);
/* the same with a second output dx2[row] = (dx[row] as stored) * scale2[row / rows_per_scale]: the DropPath-scaled copy the next
 * block of the backward chain would otherwise make in a pass of its own (timm DropPath in Block.forward: x + drop_path(f(x))) */
int ga_layernorm_bwd_dp(const void* g, const void* x, const float* mean, const float* rstd, const float* w, const void* dres,
                        void* dx, float* dw, float* db, int64_t rows, int C, int x_is_normalized, void* dx2, const float* scale2,
                        int64_t rows_per_scale, int dtype, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm2d, train mode = per-process batch statistics (ga_convnext.py:261,270,276,283,409,420).
 * The column sums come from ga_gemm's colsum/colsumsq epilogue.
 *   finalize: mean/var (biased) -> scale = w*rstd, shift = b - mean*scale; running stats updated with the unbiased
 *             variance and `momentum`; training=0 builds scale/shift from the running stats instead.
 *   affine_act: y = (x*scale[c] + shift[c]) * rowscale[row/rows_per_scale] (+ res) (ReLU)   (scale/shift/rowscale NULL ok;
 *               rowscale = the DropPath factor of the Bottleneck main branch, ga_convnext.py:310-311)
 *   bwd_reduce: s1[c] += sum g, s2[c] += sum g*xhat, g = dy * (y_relu > 0 if given) * rowscale
 *   bwd_apply:  dx = w*rstd*(g - s1/n - xhat*s2/n)
 *   With a rowscale: rows_per_scale > 0, and rows < 2^24 for affine_act / bwd_apply.  Tensors 16-byte aligned (bwd_reduce in
 *   bf16: 8-byte), column slices included; fp32 vectors 4-byte aligned.  GA_ERR_BAD_ARG otherwise, nothing is launched.
 * ------------------------------------------------------------------------------------------------------------ */
int ga_bn_finalize(const float* sum, const float* sumsq, int64_t n, const float* w, const float* b, float eps,
                   float momentum, float* running_mean, float* running_var, float* mean_out, float* rstd_out,
                   float* scale, float* shift, int C, int training, ga_stream_t stream);
/* ldx / lddx: row stride (elements) of x / dx when they are column slices of a wider matrix (the five heads'
 * gram_contraction outputs come from ONE GEMM); 0 = C.  Every other operand is contiguous [rows][C]. */
int ga_affine_act(const void* x, const float* scale, const float* shift, const void* res, const float* rowscale,
                  int64_t rows_per_scale, void* y, int64_t rows, int C, int relu, int dtype, int64_t ldx, ga_stream_t stream);
int ga_bn_bwd_reduce(const void* dy, const void* y_relu, const void* x, const float* mean, const float* rstd,
                     const float* rowscale, int64_t rows_per_scale, float* s1, float* s2, int64_t rows, int C, int dtype,
                     int64_t ldx, ga_stream_t stream);
int ga_bn_bwd_apply(const void* dy, const void* y_relu, const void* x, const float* mean, const float* rstd,
                    const float* w, const float* s1, const float* s2, const float* rowscale, int64_t rows_per_scale,
                    int64_t n, void* dx, int64_t rows, int C, int dtype, int64_t ldx, int64_t lddx, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-scale aggregate (ga_convnext.py:396-397,479-483): write pool(src) into channels [c_off, c_off+C) of the
 * concat buffer dst[B,Hout,Wout,ldd].  mode 0: f x f average (AdaptiveAvgPool2d to 14; f=1 is a copy);
 * mode 1: bilinear x2, align_corners=False (nn.Upsample).   bwd: dsrc = (dres +) pool^T(dcat slice).
 * ------------------------------------------------------------------------------------------------------------ */
int ga_pool_concat_fwd(const void* src, void* dst, int B, int Hin, int Win, int C, int Hout, int Wout, int ldd,
                       int c_off, int mode, int dtype, ga_stream_t stream);
int ga_pool_concat_bwd(const void* dcat, const void* dres, void* dsrc, int B, int Hin, int Win, int C, int Hout,
                       int Wout, int ldd, int c_off, int mode, int dtype, ga_stream_t stream);

/* Squeeze-excite (timm SEModule via create_attn('se'), ga_convnext.py:279,305):
 *   ga_spatial_sum: out[b][c] = scale * sum_hw a[b,hw,c] (* b2[b,hw,c] if given)      (fp32 [B][C])
 *   ga_se_mlp_fwd:  gate = sigmoid(W2 relu(W1 s + b1) + b2)  (W1 [R][C], W2 [C][R], fp32 master weights)
 *   ga_se_mlp_bwd:  ds = ds_scale * d(pooled mean), parameter gradients accumulated with atomics
 *   ga_chan_scale:  y[b,hw,c] = x*g[b][c] + add[b][c]   (g/add may be NULL) */
int ga_spatial_sum(const void* a, const void* b2, float* out, int B, int HW, int C, float scale, int dtype,
                   ga_stream_t stream);
int ga_se_mlp_fwd(const float* s, const float* W1, const float* b1, const float* W2, const float* b2, float* hid,
                  float* gate, int B, int C, int R, ga_stream_t stream);
int ga_se_mlp_bwd(const float* dgate, const float* gate, const float* hid, const float* s, const float* W1,
                  const float* W2, float* ds, float ds_scale, float* dW1, float* db1, float* dW2, float* db2, int B,
                  int C, int R, ga_stream_t stream);
int ga_chan_scale(const void* x, const float* g, const float* add, void* y, int B, int HW, int C, int dtype,
                  ga_stream_t stream);

/* Gram vector (GA_ConvNeXt.get_gram, ga_convnext.py:452-467; index order :424-430): the fp32 Gram matrices
 * G[B][C][C] (from ga_wgrad with Y == X) -> row-major upper-triangular entries, L2-normalised (eps 1e-12), stored in
 * the grouped layout [B][groups][Kp] (Kp >= ntri/groups, zero padded) read by the grouped embedding GEMM.
 * bwd: S[B][C][C] = symmetric gradient of the raw Gram entries (diagonal doubled) so that dX = alpha * X . S */
int ga_gram_pack_fwd(const float* G, void* out, float* inv_norm, int B, int C, int groups, int Kp, int dtype,
                     ga_stream_t stream);
int ga_gram_pack_bwd(const void* dvec, const void* vhat, const float* inv_norm, void* S, int B, int C, int groups,
                     int Kp, int dtype, ga_stream_t stream);

/* The same Gram vector through get_gram's float64 branch (`self.training and B < 128`, ga_convnext.py:456-457), straight from
 * the gram layer's NHWC output x[B][HW][C] (fp32 / bf16 per dtype) -- no ga_wgrad in front, no GEMM behind:
 *   fwd: xh = x / H rounded to the input dtype, then widened; G = xh^T xh / HW, the i <= j gather and F.normalize (eps 1e-12)
 *        in double; vec[B][groups][Kp] = the normalised vector rounded ONCE to dtype (pad columns zero).  Kept for the
 *        backward: G64[B][C (C + 1) / 2] doubles (the raw packed entries, ga_gram_f64_fwd_workspace(B, C) bytes) and
 *        inv_norm[B] doubles (1 / max(norm, 1e-12)).
 *   bwd: dvec[B][groups][Kp] widened; d_raw = (dvec - vh <vh, dvec>) / norm with vh = G64 / norm in double; the symmetric S
 *        (diagonal doubled) in `workspace` (ga_gram_f64_bwd_workspace(B, C) bytes, [B][C][C] doubles);
 *        dxh = xh . S / HW in double, cast to dtype as torch casts the float64 gradient back (bf16: through fp32), then
 *        dx[B][HW][C] = dxh / H in dtype.
 * Fixed summation order, no atomics: two runs are bit-identical.  C % 8 == 0 and C (C + 1) / 2 % groups == 0 are required. */
size_t ga_gram_f64_fwd_workspace(int B, int C);
size_t ga_gram_f64_bwd_workspace(int B, int C);
int ga_gram_f64_fwd(const void* x, void* vec, double* inv_norm, double* G64, size_t g64_bytes, int B, int HW, int C, int H,
                    int groups, int Kp, int dtype, ga_stream_t stream);
int ga_gram_f64_bwd(const void* dvec, const void* x, const double* G64, const double* inv_norm, void* dx, void* workspace,
                    size_t ws_bytes, int B, int HW, int C, int H, int groups, int Kp, int dtype, ga_stream_t stream);

/* Class attention with ONE query token (ClassAttn / LayerScaleBlockClassAttn, ga_convnext.py:153-187,244-248):
 *   token_cat: u[B][N+1][C] = cat(cls[B][C], tok[B][N][C]);  token_split: dcls (+)= du[:,0], dtok (+)= du[:,1:]
 *   class_attn: q [B][E], kv [B*(N)][2E] (k | v), E = heads*hd <= 64 per head; P fp32 [B][heads][N] saved. */
int ga_token_cat(const void* cls, const void* tok, void* u, int B, int N, int C, int dtype, ga_stream_t stream);
int ga_token_split(const void* du, void* dcls, void* dtok, int B, int N, int C, int acc_cls, int acc_tok, int dtype,
                   ga_stream_t stream);
int ga_class_attn_fwd(const void* q, const void* kv, void* out, float* P, int B, int N, int heads, int hd, float scale,
                      int dtype, ga_stream_t stream);
int ga_class_attn_bwd(const void* dout, const void* q, const void* kv, const float* P, void* dq, void* dkv, int B, int N,
                      int heads, int hd, float scale, int dtype, ga_stream_t stream);
/* split form: the class-token row and the N-1 image-token rows of k|v in separate arrays (kv_cls [B][2E], kv_tok
 * [B][N-1][2E]; N counts the class token).  The image tokens' LayerNorm (LayerScaleBlockClassAttn.norm1 on cat(x_cls, x),
 * ga_convnext.py:244-246) is row-wise, so the normalised image tokens are shared by all heads and never concatenated. */
/* tok_ld: row stride (elements) of kv_tok / dkv_tok, 0 = 2E: the five heads' k|v rows may be column slices of ONE
 * [B*(N-1)][5*2E] matrix produced by a single GEMM over the shared normalised tokens. */
int ga_class_attn_fwd2(const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, void* out, float* P, int B, int N,
                       int heads, int hd, float scale, int dtype, ga_stream_t stream);
int ga_class_attn_bwd2(const void* dout, const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, const float* P,
                       void* dq, void* dkv_cls, void* dkv_tok, int B, int N, int heads, int hd, float scale, int dtype,
                       ga_stream_t stream);

/* GA training loss, fused forward + gradient (GA/train.py:735-745):
 *   loss += sum_k L(out_k, y) + lam * sum_k KL_mean(log_softmax(out_k) || log_softmax(mean_j out_j))  (mean detached)
 *   kind 0: (label-smoothed) cross entropy; kind 1: timm BinaryCrossEntropy on smoothed one-hot targets.
 *   logits fp32 [K][B][NC]; target int64 [B]; *loss must be zeroed by the caller; dlogits (dtype) = grad * grad_scale */
int ga_loss_fwd_bwd(const float* logits, const int64_t* target, float* loss, void* dlogits, int K, int B, int NC,
                    float lam, int kind, float smoothing, float grad_scale, int dtype, ga_stream_t stream);
/* validate(): output = sum_k out_k.float(); top-k indices, ties -> lowest index  (GA/train.py:848-860).  Any 1 <= topk <= NC
 * <= 36000; a NaN sum ranks above +inf, as in torch.topk; out_sum (fp32 [B][NC]) may be NULL */
int ga_heads_topk(const float* logits, int K, int B, int NC, int topk, float* out_sum, int64_t* out_idx,
                  ga_stream_t stream);

/* Flat fused optimizer steps over fp32 [n] (train.py:769; torch.optim.SGD(nesterov) / torch.optim.AdamW semantics).
 * hp (device, fp32[8]) = {lr, weight_decay, momentum|beta1, beta2, eps, 1-beta1^t, 1-beta2^t, first_step};
 * wd_mult = 0 for the no-decay segment (timm: ndim<=1 or *.bias). */
int ga_sgd_step(float* p, const float* g, float* buf, const float* hp, int64_t n, int nesterov, float wd_mult,
                ga_stream_t stream);
int ga_adamw_step(float* p, const float* g, float* m, float* v, const float* hp, int64_t n, float wd_mult,
                  ga_stream_t stream);

/* More flat fused steps, in the same form (flat fp32 [n], hp a device fp32[8] row, wd_mult 0 for the no-decay segment; one
 * grid-stride kernel of at most 8192 x 256 threads each, no allocation, no host synchronisation, no atomics).  This comment is the
 * specification: every line is one fp32 operation order.  g' = g + wd * wd_mult * p (coupled L2 decay).
 *   ga_adam_step (torch.optim.Adam), hp = {lr, wd, beta1, beta2, eps, bc1 = 1-beta1^t, bc2 = 1-beta2^t, 0}:
 *       m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 *   ga_rmsprop_step, hp = {lr, wd, momentum, alpha, eps, 0, 0, 0}; the momentum form runs where buf is given, buf = NULL is the
 *   form without (the host passes NULL exactly when momentum is 0):
 *     tf = 0 (torch.optim.RMSprop, not centered):  sq = alpha sq + (1 - alpha) g' g';  avg = sqrt(sq) + eps;
 *       buf: buf = mu buf + g' / avg, p -= lr buf;   no buf: p -= lr g' / avg
 *     tf = 1 (timm RMSpropTF, not centered, coupled decay, lr_in_momentum):  sq += (1 - alpha) (g' g' - sq);
 *       avg = sqrt(sq + eps) -- eps INSIDE the root;   buf: buf = mu buf + lr g' / avg, p -= buf;   no buf: p -= lr g' / avg
 *       sq starts at ONE (the caller fills it; torch's starts at zero)
 *   ga_lion_step (timm Lion), hp = {lr, wd, beta1, beta2, 0, 0, 0, 0}; decoupled decay, the only step here without g':
 *       p *= (1 - lr wd wd_mult);  c = b1 m + (1 - b1) g;  p -= lr sign(c), sign(0) = 0;  m = m + (1 - b2) (g - m)
 *       (c is formed from the m the step starts with) */
int ga_adam_step(float* p, const float* g, float* m, float* v, const float* hp, int64_t n, float wd_mult,
                 ga_stream_t stream);
int ga_rmsprop_step(float* p, const float* g, float* sq, float* buf, const float* hp, int64_t n, int tf, float wd_mult,
                    ga_stream_t stream);
int ga_lion_step(float* p, const float* g, float* m, const float* hp, int64_t n, float wd_mult, ga_stream_t stream);

/* Batched variants: `jobs_dev` is a DEVICE-resident array of n descriptors (same structs as above); one launch
 * processes them all (grid.y = job).  Used for the ~270 small per-parameter jobs of a training step. */
typedef struct {
    int kind;              /* 0: y[i] += a*x[i] (n elems); 1: y[c][r] (+)= x[r][c] (x is [R][C]); 2: bias fold (R rows, C cols):
                              y[n] = rs[m]*(b[m] + sum_c x[m][c]*v[c]), m = row_perm ? row_perm[n] : n */
    float* y; const float* x; float a; int64_t n;
    int R, C, accumulate;
    const float* b; const float* rs; const float* v; const int* row_perm;
} ga_small_desc;
int ga_weight_prep_batch(const ga_wprep_desc* jobs_dev, int n, ga_stream_t stream);
int ga_weight_unfold_batch(const ga_wunfold_desc* jobs_dev, int n, ga_stream_t stream);
int ga_small_batch(const ga_small_desc* jobs_dev, int n, ga_stream_t stream);

/* LAMB (timm.optim.Lamb, the optimizer of the published GA recipes: GA/README.md:26) on the flat buffers.
 *   chunks: int32 [nchunks][4] = {element offset, length, tensor id, weight-decay flag}; a chunk never straddles a tensor.
 *   hp (device fp32[9]): lr, weight_decay, beta1, beta2, eps, 1-beta1^t, 1-beta2^t, beta3, max_grad_norm.
 *   stage1: g' = g / max(|g|_2 / max_grad_norm, 1) (|g|_2^2 = *gsumsq, from ga_sumsq_f32); m, v updated;
 *           u = (m/bc1) / (sqrt(v)/sqrt(bc2) + eps) + wd*p;  norms[2t] += sum p^2, norms[2t+1] += sum u^2 (caller zeroes norms)
 *   stage2: p -= lr * trust_t * u, trust_t = |p_t| / |u_t| where weight decay applies (both > 0), else 1. */
int ga_lamb_stage1(const float* p, const float* g, float* m, float* v, float* u, const float* hp, const float* gsumsq,
                   const int* chunks, int nchunks, float* norms, ga_stream_t stream);
int ga_lamb_stage2(float* p, const float* u, const float* hp, const int* chunks, int nchunks, const float* norms,
                   ga_stream_t stream);

/* LARS (timm.optim.Lars; always_adapt is not built) over LAMB's chunk table (one workgroup per chunk, the caller zeroes norms).
 *   stage1: norms[2t] += sum p^2, norms[2t+1] += sum g^2 per tensor t.  Each workgroup adds its two partial sums with ONE atomic
 *           each, as ga_lamb_stage1 does: a tensor of several chunks has its partials added in the order the workgroups arrive, so
 *           two runs on the same inputs may differ in the last bits of its norms (and, through the trust ratio, of buf and p); a
 *           tensor of one chunk is bit-reproducible.
 *   stage2: hp (device fp32[8]) = {lr, wd, momentum, trust_coeff, eps, first_step, 0, 0}; the momentum form runs where buf is given
 *           (buf = NULL exactly when momentum is 0).  A chunk is ADAPTED where its decay flag is set and wd != 0 (timm adapts only
 *           where the group's weight_decay != 0):
 *             w = sqrt(norms[2t]), q = sqrt(norms[2t+1]);  trust = trust_coeff w / (q + w wd + eps) where w > 0 and q > 0, else 1;
 *             trust_clip: trust = min(trust / lr, 1);  d = (g + wd p) trust
 *           every other chunk: d = g.  Then SGD momentum with dampening 0:
 *             buf = first_step ? d : mu buf + d;  d = nesterov ? d + mu buf : buf;  p -= lr d        (no buf: p -= lr d) */
int ga_lars_stage1(const float* p, const float* g, const int* chunks, int nchunks, float* norms, ga_stream_t stream);
int ga_lars_stage2(float* p, const float* g, float* buf, const float* hp, const int* chunks, int nchunks, const float* norms,
                   int nesterov, int trust_clip, ga_stream_t stream);

/* gradient clipping on the flat fp32 gradient buffer (timm dispatch_clip_grad via NativeScaler, GA/train.py:312-333):
 *   ga_sumsq_f32: *out += sum x^2 (caller zeroes *out; under DDP call after the all-reduce);
 *   ga_clip_grad_f32 mode 0 ('norm'): g *= min(1, limit / (sqrt(*sumsq) + 1e-6));  mode 1 ('value'): clamp to [-limit, limit] */
int ga_sumsq_f32(const float* x, int64_t n, float* out, ga_stream_t stream);
int ga_clip_grad_f32(float* g, int64_t n, const float* sumsq, float limit, int mode, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * GA-CSWin: cross-shaped stripe-window attention with LePE (LePEAttention.forward, ga_cswin.py:110-136; get_lepe
 * :95-108; img2windows / windows2img :215-233) for the 1 or 2 branches of a CSWinBlock (:202-207) in ONE launch.
 *   qkv [B*L][ldq]: q | k | v column blocks of width C (tokens in image raster order, L = reso*reso);
 *   branch i owns channels [i*C/nbranch, (i+1)*C/nbranch) of each block, heads/nbranch heads, stripes Hs[i] x Ws[i];
 *   out[b, t, ch] = softmax_j((q_t * scale) . k_j) v_j + conv3x3_depthwise(v)(t)   over the tokens j of t's stripe,
 *   the 3x3 (lepe_w[i]: fp32 [C/nbranch][9] = get_v.weight, lepe_b[i]) zero padded at the STRIPE border.
 *   head_dim in {8, 16, 32}; Hs*Ws <= 128, for fwd AND bwd at every head_dim and dtype (both take their LDS size from one host
 *   function and refuse with GA_ERR_BAD_ARG what exceeds 160 KiB; no accepted shape does: where the generic backward's two
 *   [N][N+1] score planes do not fit -- head_dim 32: N > 109, head_dim 16: N > 126 -- it keeps one and recomputes P).
 *   bf16 with head_dim 32 and Hs*Ws <= 112 runs on MFMA, everything else on a generic fp32 form.
 * bwd: dqkv [B*L][ldq] = d(q | k | v) from dout [B*L][ldo]  (dv includes the LePE transpose).  With a caller-owned `lepe_ws` of
 *   ga_cswin_attn_bwd_workspace(d) bytes (16-byte aligned; 0 = this shape runs the generic form, pass NULL) the kernel also
 *   leaves the per-(window, head) partial LePE weight gradients there from the tiles it already holds in LDS;
 *   ga_cswin_lepe_wgrad_reduce then adds their sum into dw_i / db_i.  The buffer may be reused once the reduce has run.
 * lepe_wgrad: the unfused form of the same (any shape): dw_i[ch][tap] += sum dout * shifted v, db_i[ch] += sum dout  (fp32 atomics). */
typedef struct {
    int B, reso, C, heads, nbranch;
    int Hs[2], Ws[2];
    const float* lepe_w[2];
    const float* lepe_b[2];
    float scale;
    int dtype;
    const void* qkv; int64_t ldq;
    void* out; int64_t ldo;
} ga_cswin_attn_desc;
int ga_cswin_attn_fwd(const ga_cswin_attn_desc* d, ga_stream_t stream);
size_t ga_cswin_attn_bwd_workspace(const ga_cswin_attn_desc* d);
int ga_cswin_attn_bwd(const ga_cswin_attn_desc* d, const void* dout, void* dqkv, void* lepe_ws, size_t ws_bytes, ga_stream_t stream);
int ga_cswin_lepe_wgrad_reduce(const ga_cswin_attn_desc* d, const void* lepe_ws, float* dw0, float* db0, float* dw1, float* db1,
                               ga_stream_t stream);
int ga_cswin_lepe_wgrad(const ga_cswin_attn_desc* d, const void* dout, float* dw0, float* db0, float* dw1, float* db1,
                        ga_stream_t stream);
/* deep-stem helpers (ga_cswin.py:463-477):
 *   ga_nchw3_to_nhwc8: fp32 NCHW [B,3,H,W] -> NHWC [B,H,W,8] in `dtype`, channels 3..7 zero (the first 3x3/s2 conv then is
 *                      a GA_A_CONV3S2 gather with C = 8);
 *   ga_convw_pack:     fp32 [Co][Ci][taps] -> out[co][tap*Cp + ci] in `dtype` (zero for ci >= Ci and up to ldo);
 *   ga_convw_unpack_grad: dW[co][ci][tap] += G[co][tap*Cp + ci];
 *   ga_conv3s2_dgrad_prep: fp32 [Co][Ci][3][3] -> out[(py,px,ci)][(ay,ax,co)] (4*Ci rows, ldo >= 4*Co), see GA_A_NEIGH2 */
/* LayerNorm(affine) -> GELU(erf) between the stem convs (ga_cswin.py:466-468,471-473): y = gelu(LN(x)*w + b);
 * bwd: dx = LN'(g * gelu'(LN(x)*w + b)), dw / db accumulated (fp32 atomics).  C a power of two in [8, 512]. */
int ga_layernorm_gelu_fwd(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd, int64_t rows,
                          int C, float eps, int dtype, ga_stream_t stream);
int ga_layernorm_gelu_bwd(const void* g, const void* x, const float* mean, const float* rstd, const float* w, const float* b,
                          void* dx, float* dw, float* db, int64_t rows, int C, int dtype, ga_stream_t stream);
int ga_nchw3_to_nhwc8(const float* x, void* y, int B, int H, int W, int dtype, ga_stream_t stream);
int ga_convw_pack(const float* w, void* out, int Co, int Ci, int taps, int Cp, int64_t ldo, int dtype, ga_stream_t stream);
int ga_convw_unpack_grad(const float* G, float* dW, int Co, int Ci, int taps, int Cp, int64_t ldg, ga_stream_t stream);
int ga_conv3s2_dgrad_prep(const float* w, void* out, int Co, int Ci, int64_t ldo, int dtype, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * MAP head (MAP/models/map.py).  The GEMM-shaped parts go through ga_gemm / ga_wgrad; these are the rest.
 *   ga_gram_pack_fwd2 / _bwd2: ga_gram_pack_* with GramToken's token interleave (map.py:225-227): packed upper-triangular
 *       entry t is stored at (t % ntok) * (ntri / ntok) + t / ntok before the grouped layout is applied (ntok = 1: identity).
 *   ga_map_tokens_fwd: e [B][C*T] (channel c*T + t, the bp_reduction output, map.py:231-232) -> tok [B][T (+1)][C];
 *       add_mean: the extra row is the mean over the T tokens (CAP's self-distillation token, map.py:273-275).  _bwd: its transpose.
 *   ga_class_attn_mt_*: ClassAttention with 1 <= T <= 8 query tokens (map.py:118-144, in_dim == dim branch; `interactive`: ga_class_attn_mt_ia_* below):
 *       q [B][T][E], kv_cls [B][T][2E] (k | v of the class rows), kv_tok = k | v rows of the N - T >= 1 image tokens (row stride
 *       tok_ld); P [B][T][heads][N] fp32 = softmax, saved; mask (fp32, same shape, or NULL) = attention dropout mask
 *       (already divided by keep); out [B][T][E].  bwd overwrites dq, dkv_cls and the dkv_tok rows (stride dtok_ld).
 *       Requires hd % 8 == 0, E = heads * hd <= 512, tok_ld / dtok_ld >= 2E and multiples of 8, q, kv_cls, kv_tok (and in _bwd
 *       dout, dkv_cls, dkv_tok) 16-byte aligned, and an LDS working set of at most 160 KiB:
 *       4 (N E / 8 + c T heads N + 16 E) bytes, c = 1 forward, 2 backward.  GA_ERR_BAD_ARG otherwise, nothing is launched.
 *   ga_map_loss_fwd_bwd: MAP/train.py:792-839 (distill_tokens == 0): ga_loss_fwd_bwd on the org logits plus, per group,
 *       KL_sum(log_softmax(avg_k) || log_softmax(org_k).detach()) / (B*NC); davg = its gradient (avg == NULL: the GA loss).
 *   ga_gelu_fwd / _bwd: y = gelu(x) (erf), dx = dy * gelu'(x)   (MultiScale ConvNormAct with non_linearity = GELU, map.py:331)
 *   ga_relu_drop: out = a * m, deriv = (a > 0) * m  for a = relu output, m = fp32 dropout mask or NULL (GroupConvMlp, act ReLU)
 *   ga_mask_mul: y = x * m (+ res);   ga_copy2d: dst[r][0..cols) (+)= src[r][0..cols) with row strides (elements) */
int ga_gram_pack_fwd2(const float* G, void* out, float* inv_norm, int B, int C, int groups, int Kp, int ntok, int dtype,
                      ga_stream_t stream);
int ga_gram_pack_bwd2(const void* dvec, const void* vhat, const float* inv_norm, void* S, int B, int C, int groups, int Kp,
                      int ntok, int dtype, ga_stream_t stream);
int ga_map_tokens_fwd(const void* e, void* tok, int B, int C, int T, int add_mean, int dtype, ga_stream_t stream);
int ga_map_tokens_bwd(const void* dtok, void* de, int B, int C, int T, int add_mean, int dtype, ga_stream_t stream);
int ga_class_attn_mt_fwd(const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, void* out, float* P,
                         const float* mask, int B, int T, int N, int heads, int hd, float scale, int dtype, ga_stream_t stream);
int ga_class_attn_mt_bwd(const void* dout, const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, const float* P,
                         const float* mask, void* dq, void* dkv_cls, void* dkv_tok, int64_t dtok_ld, int B, int T, int N,
                         int heads, int hd, float scale, int dtype, ga_stream_t stream);
/* ClassAttention with `interactive` = True (map.py:96-98,130-136): W1, W2 [heads][heads] + b1, b2 [heads] fp32 mix the HEADS of
 * the scores before and of the probabilities after the softmax: U = S + W1 S + b1, A = softmax(U), Pm = A + W2 A + b2.
 * out = (Pm * mask) v.  Same operand layouts as ga_class_attn_mt_*; P saves A.  _bwd overwrites dq, dkv_cls and the dkv_tok rows
 * and ACCUMULATES dW1, db1, dW2, db2 (fp32 atomics: the caller zeroes them).  These kernels access every operand element by
 * element, so their requirements are weaker than the plain pair's: 1 <= T <= 8, N > T, any heads, hd >= 1 (hd % 8 and E <= 512
 * are NOT required), tok_ld / dtok_ld >= 2E with no multiple-of-8 rule, pointers aligned to their element type only, and an LDS
 * working set of at most 160 KiB: 4 * 2 heads N bytes forward, 4 (2T + 4) heads N bytes backward.  GA_ERR_BAD_ARG otherwise. */
int ga_class_attn_mt_ia_fwd(const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, void* out, float* P,
                            const float* mask, const float* W1, const float* b1, const float* W2, const float* b2, int B, int T, int N,
                            int heads, int hd, float scale, int dtype, ga_stream_t stream);
int ga_class_attn_mt_ia_bwd(const void* dout, const void* q, const void* kv_cls, const void* kv_tok, int64_t tok_ld, const float* P,
                            const float* mask, const float* W1, const float* W2, const float* b2, void* dq, void* dkv_cls,
                            void* dkv_tok, int64_t dtok_ld, float* dW1, float* db1, float* dW2, float* db2, int B, int T, int N,
                            int heads, int hd, float scale, int dtype, ga_stream_t stream);
int ga_map_loss_fwd_bwd(const float* org, const float* avg, const int64_t* target, float* loss, void* dorg, void* davg, int K,
                        int B, int NC, float lam, int kind, float smoothing, float grad_scale, int dtype, ga_stream_t stream);
/* the same losses on DENSE targets [B][NC] fp32 (mixup / cutmix, GA/train.py:616-621: SoftTargetCrossEntropy for kind 0 --
 * mean_b sum_c -t log_softmax(x) -- and BinaryCrossEntropy on the mixed targets for kind 1); exactly one of `target` (class
 * indices, with `smoothing`) and `dense` is given; bce_threshold >= 0 binarises the BCE target (--bce-target-thresh), < 0: off.
 * avg / davg as ga_map_loss_fwd_bwd (NULL for the GA loss). */
int ga_loss_dense_fwd_bwd(const float* org, const float* avg, const int64_t* target, const float* dense, float* loss, void* dorg,
                          void* davg, int K, int B, int NC, float lam, int kind, float smoothing, float bce_threshold,
                          float grad_scale, int dtype, ga_stream_t stream);
/* timm JsdCrossEntropy (--aug-splits S --jsd-loss, GA/train.py:559-561,613-615) in place of the per-head loss, fused with the same
 * head-decorrelation and self-distillation terms as ga_map_loss_fwd_bwd.  The batch is split-major: row i + s Bs is split s of base
 * sample i, Bs = B / num_splits; only target[0 .. Bs) is read.  With p_s = softmax of the rows of split s, per head:
 *     CE_smooth(x_0, y) (mean over Bs; on = 1 - smoothing + smoothing / NC, off = smoothing / NC)
 *   + alpha / S * sum_s (1 / Bs) sum_ic p_s (log p_s - log m),   m = clamp(mean_s p_s, 1e-7, 1)
 *   + lam * KL_mean(log_softmax(out_k) || log_softmax(mean_j out_j).detach())  and, with avg, the self-distillation term: both over
 *     all B rows, as in ga_loss_fwd_bwd / ga_map_loss_fwd_bwd.
 * Gradient of the JSD term, A = alpha / B:  g_sc = A [ (log p_sc - log m_c) + (mean_s p_sc outside [1e-7, 1] ? 1 : 0) ],
 *     d / dx_sc = p_sc (g_sc - sum_c' p_sc' g_sc'): the clamp passes no gradient outside its range, and passes it at equality.
 * Same conventions as ga_loss_dense_fwd_bwd: org / avg fp32 [K][B][NC]; avg, dorg, davg may be NULL; the loss is ADDED to *loss
 * (the caller zeroes it) and not scaled; dorg / davg in `dtype` = gradient * grad_scale, every element written once, by one
 * rounding of an fp32 value; no atomics but the one addition per workgroup onto *loss.
 * Deviation from autograd: log p is formed as x - logsumexp(x), never as log(p), so where a probability underflows to 0 the term
 * and its gradient are their limit 0 and the rest of the row stays finite (torch's xlogy derivative gives NaN = 0 / 0 there).
 * One workgroup per base sample holds the log-softmax of the head-mean row of each of its S rows in LDS: 4 (S NC + 8) bytes, at
 * most 160 KiB (S NC <= 40952).  GA_ERR_BAD_ARG, nothing launched: num_splits < 2 or > 8, B % num_splits != 0, K / B / NC < 1, a
 * NULL org / target / loss, davg without avg, or the LDS bound. */
int ga_loss_jsd_fwd_bwd(const float* org, const float* avg, const int64_t* target, float* loss, void* dorg, void* davg, int K, int B,
                        int NC, int num_splits, float lam, float smoothing, float alpha, float grad_scale, int dtype,
                        ga_stream_t stream);
/* timm.data.Mixup (mode 'batch') on the device, lam / box drawn by the host as timm does (GA/train.py:544-557,727-728):
 *   ga_mixup_batch:  fp32 NCHW x -> out (out of place): mixup out[b] = x[b]*lam + x[B-1-b]*(1-lam), or cutmix (x[B-1-b] inside
 *                    the box [yl,yh) x [xl,xh));
 *   ga_mixup_target: class indices -> dense [B][NC]: lam * onehot_s(t[b]) + (1-lam) * onehot_s(t[B-1-b]).
 * lam / smoothing are doubles: 1 - lam and the on / off values are formed in double and rounded to fp32 once, as torch does. */
int ga_mixup_batch(const float* x, float* out, int B, int CH, int H, int W, double lam, int cutmix, int yl, int yh, int xl, int xh,
                   ga_stream_t stream);
int ga_mixup_target(const int64_t* target, float* out, int B, int NC, double lam, double smoothing, ga_stream_t stream);
/* uint8 NCHW batch (timm fast_collate) -> fp32 NCHW, out = (x - mean[c]) / std[c]; mean / std are HOST arrays of CH <= 4 floats
 * (already scaled by 255 as timm's PrefetchLoader holds them, GA/train.py:567-595); H*W a multiple of 4 */
int ga_u8_normalize(const void* x, float* out, int B, int CH, int H, int W, const float* mean, const float* std, ga_stream_t stream);
/* timm RandomErasing as PrefetchLoader runs it: on the device, on the normalised batch, ahead of mixup (MAP/train.py:214-220,
 * 643-646).  One out-of-place pass: out = ga_u8_normalize(x) (x_is_u8; same arithmetic, bit-identical) or a copy of the fp32 x,
 * except inside the boxes of a sample, where it is the fill.  boxes: DEVICE int32 [B][max_count][4] = top, left, h, w, drawn by the
 * host (imagenet_models_amd.RandomErasing); h == 0: unused slot; where boxes of a sample overlap the later one wins.
 * mode 0 'const': zeros; 1 'rand': one N(0,1) colour per (box, channel); 2 'pixel': N(0,1) per element.  H*W % 4 == 0.
 * The normals are a pure function of (seed, offset, index) -- no state, no atomics, independent of the launch shape:
 *   Philox4x32-10, key = (seed[31:0], seed[63:32]), counter = (q[31:0], q[63:32], offset[31:0], offset[62:32] | stream << 31);
 *   pixel (stream 0): q = i >> 2 for the flat element index i = ((b*CH + c)*H + y)*W + x, element i takes normal n[i & 3];
 *   rand (stream 1): q = (b*max_count + j)*CH + c for box j, the colour is n[0];
 *   uniforms u_k = ((r_k >> 9) + 0.5) * 2^-23 of the outputs r0..r3 (never 0: no log(0));
 *   n0 = R(u0) cos(2 pi u1), n1 = R(u0) sin(2 pi u1), n2 = R(u2) cos(2 pi u3), n3 = R(u2) sin(2 pi u3), R(u) = sqrt(-2 ln u).
 * A caller advances `offset` (< 2^63) by one per step for fresh noise from one seed. */
int ga_input_erase(const void* x, int x_is_u8, float* out, int B, int CH, int H, int W, const float* mean, const float* std,
                   const int32_t* boxes, int max_count, int mode, uint64_t seed, uint64_t offset, ga_stream_t stream);
/* timm's collate-time order -- FastCollateMixup on the uint8 batch, PrefetchLoader's normalisation, RandomErasing last on the mixed
 * image (what every recipe with the prefetcher runs) -- as ONE out-of-place pass over the batch.  The partner of sample b is
 * B-1-b (B even); every read is of the original x.  mix: DEVICE int32 [B][8], one 32-byte row per sample, drawn by the host
 * (imagenet_models_amd.FastCollateMixup), so timm's modes 'batch', 'elem' and 'pair' are the same kernel:
 *   { kind, yl, yh, xl, xh, bits(l), bits(m), 0 }     kind 0 none, 1 mixup, 2 cutmix;  l = fp32 lam, m = its fp32 complement
 *   (numpy forms m as float32(1.0 - lam) for a scalar lam and as float32(1) - l for a lam vector: an ulp apart, so both travel)
 *   none:   the sample's own value
 *   mixup:  u8(rint(fl(fl(a*l) + fl(b*m))))  a = own byte, b = the partner's; three separately rounded fp32 operations (no FMA),
 *           rint = round half to even (np.rint)
 *   cutmix: the partner's value inside [yl, yh) x [xl, xh), the own one outside; an empty box is legal.  0 <= yl <= yh <= H and
 *           0 <= xl <= xh <= W are the host's responsibility: the kernel clamps nothing.
 * The mixed byte is then normalised with ga_u8_normalize's arithmetic and erased with ga_input_erase's: boxes / max_count / mode /
 * seed / offset and the Philox counter layout are those of ga_input_erase (the noise index is the flat index of the OUTPUT element);
 * boxes NULL or max_count 0: no erase.  The result equals ga_input_erase run on the separately mixed uint8 batch, bit for bit.
 * x_is_u8 == 0: timm's Mixup on an fp32 batch -- the same blend without the rounding to integers, the box copy, no normalisation.
 * GA_ERR_BAD_ARG: odd B, out == x, H*W % 4 != 0, x not 4 (uint8) / 16-byte aligned, out / mix / boxes not 16-byte aligned, and the
 * limits of ga_input_erase.
 *   ga_mixup_target_elem: class indices -> dense [B][NC] for a DEVICE fp32 lam[B]: row b = y1 * lam[b] + y2 * (1 - lam[b]), y2 from
 *   target[B-1-b]; on / off are formed in double and rounded once; complement, products and sum are separate fp32 roundings. */
int ga_input_collate(const void* x, int x_is_u8, float* out, int B, int CH, int H, int W, const float* mean, const float* std,
                     const int32_t* mix, const int32_t* boxes, int max_count, int mode, uint64_t seed, uint64_t offset,
                     ga_stream_t stream);
int ga_mixup_target_elem(const int64_t* target, float* out, int B, int NC, const float* lam, double smoothing, ga_stream_t stream);
/* timm RandAugment (--aa rand-mN-mstd0.5-inc1, every recipe of MAP/train_with_script.py:13-19) on the uint8 NCHW batch of timm's
 * fast_collate, ahead of ga_input_collate / ga_input_erase / ga_u8_normalize: out-of-place, CH == 3, every byte equal to what PIL
 * gives for the call timm makes.  ops: DEVICE table [B][n_layers] of 64-byte rows, drawn by the host (imagenet_models_amd.RandAugment):
 *   { int32 kind, int32 interp, int32 iarg, fp32 farg, double m[6] }
 * Layer l+1 of a sample reads the COMPLETE output of layer l.  n_layers == 0 and a row of kind 0 copy the sample; the kernel treats
 * an unknown kind as 0 (ga_rand_augment_check_table refuses one on the host, before the table is staged).
 *   kind 0 none
 *        1 autocontrast  per channel: lo / hi = lowest / highest occupied histogram bin; hi <= lo: identity; else
 *                        lut[i] = clamp(int(i * s + (-lo * s)), 0, 255), s = 255.0 / (hi - lo), in double, truncated toward zero
 *        2 equalize      per channel, histogram h: step = (sum(h) - h[last occupied bin]) / 255 (integer); <= 1 occupied bin or
 *                        step == 0: identity; else n = step / 2; for i = 0..255: lut[i] = min(255, n / step); n += h[i]
 *        3 invert        255 - a
 *        4 posterize     a & ~(2^(8 - iarg) - 1);  iarg >= 8: identity;  iarg 0: 0
 *        5 solarize      a < iarg ? a : 255 - a
 *        6 solarize_add  a < 128 ? min(255, a + iarg) : a
 *        7 color         blend(gray, a, farg)        gray = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 of the pixel
 *        8 contrast      blend(mean, a, farg)        mean = int(sum(gray over the image) / (H * W) + 0.5), the division in double
 *        9 brightness    blend(0, a, farg)
 *       10 sharpness     blend(smooth, a, farg)      smooth = the 3x3 kernel (1,1,1,1,5,1,1,1,1): the fp32 sum / 13, + 0.5, clipped and
 *                                                    truncated; the border row and column are the image's own
 *       11 affine        m, interp (PIL's codes: 0 nearest, 2 bilinear, 3 bicubic); a pixel without a source takes fill[c]
 *   blend(d, a, f) = d + f * (a - d) in fp32, the product and the sum separately rounded (no FMA); <= 0 -> 0, >= 255 -> 255, else
 *   TRUNCATED.
 *   affine, output pixel (x, y), bilinear / bicubic, all in double without contraction:
 *     xin = m0 (x + 0.5) + m1 (y + 0.5) + m2,  yin = m3 (x + 0.5) + m4 (y + 0.5) + m5;  outside 0 <= xin < W, 0 <= yin < H: fill
 *     x' = xin - 0.5, x0 = floor(x'), dx = x' - x0 (likewise y); neighbour indices are clamped to the image
 *     bilinear: L(v1, v2, d) = v1 + (v2 - v1) d along x for two rows, then along y
 *     bicubic, taps x0-1 .. x0+2: p1 = v2; p2 = -v1 + v3; p3 = 2 (v1 - v2) + v3 - v4; p4 = -v1 + v2 - v3 + v4;
 *               p1 + d (p2 + d (p3 + d p4)) along x for four rows, then along y
 *     result <= 0 -> 0, >= 255 -> 255, else truncated
 *   affine, nearest -- PIL leaves the double path here, and so does this:
 *     m1 == 0 and m3 == 0: xo = m2 + m0 * 0.5, then x additions of m0 (each rounded); source column int(xo), none if xo < 0 or >= W;
 *                          rows likewise from m5 + m4 * 0.5 and m4
 *     otherwise 16.16 fixed point, F(v) = floor(v * 65536 + 0.5): source column (F(m2 + m0 * 0.5 + m1 * 0.5) + F(m1) y + F(m0) x) >> 16,
 *                          row (F(m5 + m3 * 0.5 + m4 * 0.5) + F(m4) y + F(m3) x) >> 16, none outside the image
 * fill: HOST array of CH bytes.  work: caller-owned, ga_rand_augment_work_bytes(...) bytes: 1 KiB of per-sample statistics (the
 * three LUTs, the grey mean) and the ping-pong image(s) between layers (none for n_layers <= 1, one for 2, two beyond).
 * No allocation, no host synchronisation, no floating-point atomics (integer LDS histograms only): deterministic.
 * GA_ERR_BAD_ARG, nothing launched: out == x, CH != 3, H*W % 4 != 0, H or W >= 32768, x / out off the 4-byte or ops / work off the
 * 16-byte grid, work_bytes too small, n_layers < 0; from ga_rand_augment_check_table (a HOST copy of `rows` table rows): a kind
 * outside 0..11 or an interp other than 0, 2, 3. */
int ga_rand_augment(const void* x, void* out, void* work, size_t work_bytes, int B, int CH, int H, int W, const void* ops, int n_layers,
                    const uint8_t* fill, ga_stream_t stream);
size_t ga_rand_augment_work_bytes(int B, int CH, int H, int W, int n_layers);
int ga_rand_augment_check_table(const void* ops_host, int rows);
/* The first step of every recipe's input stage, on DECODED images: timm's RandomResizedCropAndInterpolation + RandomHorizontalFlip
 * (training, GA/train.py:195-217 through create_loader) and Resize(floor(img / crop_pct)) + CenterCrop (evaluation), which timm runs
 * on the host, per image, with PIL's antialiased resize.  Every output byte equals what PIL gives for the calls timm and torchvision
 * make: img.crop(box).resize((vw, vh), code), transpose(FLIP_LEFT_RIGHT), the centre window.
 * src: one DEVICE byte buffer of src_bytes bytes holding RGB images back to back, interleaved HWC as a decoder produces them, row
 * pitch 3 * src_w bytes without padding (rows are in general not 4-byte aligned).  out: the uint8 NCHW (B, 3, OH, OW) batch of timm's
 * fast_collate -- what ga_rand_augment, ga_input_collate, ga_input_erase and ga_u8_normalize take; the HWC -> CHW transpose is part
 * of the pass.  rows: DEVICE table of one 64-byte row per sample, drawn by the host (imagenet_models_amd.RandomResizedCrop /
 * ResizeCenterCrop):
 *   { int64 src_off; int32 src_h, src_w;   image b starts at src + src_off
 *     int32 top, left, h, w;               crop box; the resample sees ONLY the box (crop first, then resize: taps clamp at the box edge)
 *     int32 vh, vw;                        size the box is resized to
 *     int32 oy, ox;                        window of that resized image written to out: rows oy..oy+OH-1, columns ox..ox+OW-1
 *     int32 interp;                        PIL code: 2 bilinear, 3 bicubic
 *     int32 flip;                          1: mirror left-right after the resize (ahead of the window)
 *     int32 pad[2]; }
 * Training: vh, vw = OH, OW and oy = ox = 0.  Evaluation: the box is the whole image, (vh, vw) the short-side-scaled size and
 * (oy, ox) the centre crop.
 * The arithmetic is PIL's ImagingResample for 8-bit channels.  Per axis, in = the box extent, out = vw or vh, everything in double,
 * every operation separately rounded (no FMA), in the order written:
 *   scale = in / out;  fs = max(scale, 1.0);  support = S * fs, S = 1 bilinear, 2 bicubic;  ss = 1.0 / fs
 *   output index xx:  center = (xx + 0.5) * scale
 *                     xmin = max(0, (int)(center - support + 0.5));  xmax = min(in, (int)(center + support + 0.5))
 *                     tap x in [xmin, xmax):  w_x = f((x - center + 0.5) * ss)
 *                     ww = the sum of the w_x in ascending x;  w_x = w_x / ww (a true division; skipped if ww == 0)
 *                     coefficient = (int)(-0.5 + w_x * 2^22) for w_x < 0, (int)(0.5 + w_x * 2^22) otherwise
 *   f bilinear, t = |t|:  1.0 - t for t < 1, else 0
 *   f bicubic, a = -0.5:  ((a + 2.0) * t - (a + 3.0)) * t * t + 1 for t < 1;  (((t - 5) * t + 8) * t - 4) * a for t < 2;  else 0
 *   output byte = clamp((2^21 + sum pixel * coefficient) >> 22, 0, 255), the sum in int32, the shift arithmetic.
 * The horizontal pass runs first and is rounded to uint8; the vertical pass runs on those bytes.  PIL skips a pass whose size does
 * not change: its coefficients are exactly one tap of 2^22, so running it gives the same bytes, and it is run.
 * The coefficients are computed on the device, per output column and row of the window; ga_resample_coeffs writes one axis of them
 * with the same device function: DEVICE bounds[out_size][2] = (xmin, count) and coeffs[out_size][ksize], zero past count
 * (ksize >= min(in_size, (int)ceil(support) * 2 + 1), PIL's row pitch).
 * work: caller-owned, ga_resize_crop_work_bytes(HOST copy of the table, ...) bytes: B + 1 region offsets, then per sample its
 * coefficients and bounds and the planar [3][h][OW] bytes between the passes.  No tap count is capped, no LDS tile is used, no
 * allocation, no host synchronisation, no atomics: the result does not depend on the launch shape.
 * GA_ERR_BAD_ARG, nothing launched -- from ga_resize_crop_check_table, on a HOST copy of the table before it is staged: a box outside
 * its image or h or w below 1; src_off + 3 * src_h * src_w > src_bytes; a window outside (vh, vw); interp not 2 or 3; flip not 0 or
 * 1; any extent at or above 32768; OW % 4 != 0 -- and from ga_resize_crop itself: the same limits on B, OH and OW; out, rows or work
 * off the 16-byte grid; work_bytes below what a table of one-pixel boxes needs.  The kernels clamp nothing and read nothing outside
 * a box: a table that fails the check must never reach them.  (A workspace smaller than the DEVICE table needs cannot be seen by the
 * host: the launches then write nothing but the region offsets.) */
int ga_resize_crop(const void* src, uint64_t src_bytes, const void* rows, void* out, void* work, size_t work_bytes, int B, int OH, int OW,
                   ga_stream_t stream);
size_t ga_resize_crop_work_bytes(const void* rows_host, int B, int OH, int OW);
int ga_resize_crop_check_table(const void* rows_host, int B, int OH, int OW, uint64_t src_bytes);
int ga_resample_coeffs(int in_size, int out_size, int interp, int32_t* bounds, int32_t* coeffs, int ksize, ga_stream_t stream);
/* Baseline JPEG files into the byte buffer ga_resize_crop reads: the decoder ahead of the input stage.  The entropy stage runs on the
 * host, per file and thread-safe (csrc/jpeg_host.h: plain C++, no device call, no allocation, no global state); the pixel
 * reconstruction runs on the device and equals PIL 12.2 / libjpeg-turbo -- Image.open(f).convert('RGB') -- byte for byte.
 * ga_jpeg_probe and ga_jpeg_entropy_decode return 0 OK, 1 UNSUPPORTED (a valid file of another kind, or no JPEG at all: hand it to
 * another decoder), 2 CORRUPT; GA_ERR_BAD_ARG for a null pointer.  They never read past bytes + n nor write past coef_capacity.
 *   OK: SOF0, or SOF1 with 8-bit samples; Huffman coded; ONE interleaved scan (Ss 0, Se 63, Ah = Al = 0) with the components in frame
 *   order; 1 component sampled 1 x 1, or 3 components that libjpeg takes for YCbCr (a JFIF marker, or an Adobe marker with transform
 *   1, or neither and ids other than 'R' 'G' 'B') with the luma sampled 1 x 1, 2 x 1 or 2 x 2 and both chroma 1 x 1; DQT of 8 or 16
 *   bits with entries up to 32767 (libjpeg's multipliers are signed 16-bit words); DRI / RSTn; width and height below 32768.
 *   UNSUPPORTED: progressive, arithmetic, lossless, 12-bit, 4 components, RGB-coded, any other sampling, several scans, a height of
 *   0 (DNL), a missing table, larger extents.  CORRUPT: a header that ends early or contradicts itself, a Huffman table with more
 *   codes than a length holds, and in the scan: the data ends or a marker appears inside a block, a code no symbol has, a run past
 *   coefficient 63, anything but the expected RSTn at a restart interval.
 * info[24] (int64): 0 width, 1 height, 2 components, 3 hmax, 4 vmax, 5 the int16 coefficients of the image, 6 restart interval,
 *   7 MCUs per row, 8 MCU rows; component c: 9 + 4c .. 12 + 4c = h, v, blocks_w, blocks_h over the MCU-padded grid; 21 + c: its start
 *   in the coefficient buffer.
 * coef: QUANTISED coefficients, int16, natural (de-zigzagged) order, per component [blocks_h][blocks_w][64], the components back to
 *   back; qt: 3 x 64 uint16, the table of component c at 64 c, natural order.  Both caller-owned (slices of a pinned staging buffer).
 * ga_jpeg_reconstruct: DEVICE table of one 64-byte row per image
 *   { int64 coef_off;  int16 units into coef      int64 dst_off;  bytes into dst      int64 work_off;  bytes into work
 *     int32 qt_off;    uint16 units into qt       int32 width, height, ncomp;         int32 hs, vs;    the luma sampling
 *     int32 mcus_w, mcus_h;                       int32 pad[2]; }
 * dst: the RaggedBatch byte buffer: image i is uint8 [height][width][3] at dst_off (a multiple of 16), rows unpadded; a grey image
 * writes Y to all three channels; no byte outside the images is written.  work: ga_jpeg_work_bytes(HOST table) bytes, one byte per
 * coefficient: the components' planes over the MCU-padded grid between the two launches; work_off is the host's (regions back to back).
 * The arithmetic, all shifts arithmetic, every intermediate of the IDCT 64-bit:
 *   dequantise   x = coef * qt
 *   IDCT         jidctint "islow", CONST_BITS 13, PASS1_BITS 2.  One 1-D pass on i0..i7:
 *                  z1 = (i2 + i6) 4433; t2 = z1 - i6 15137; t3 = z1 + i2 6270; t0 = (i0 + i4) << 13; t1 = (i0 - i4) << 13
 *                  t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
 *                  a0..a3 = i7, i5, i3, i1; z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3; z5 = (z3 + z4) 9633
 *                  a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995
 *                  z3 = z3 (-16069) + z5; z4 = z4 (-3196) + z5; a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4
 *                  out 0/7 = t10 +- a3, 1/6 = t11 +- a2, 2/5 = t12 +- a1, 3/4 = t13 +- a0, each (x + (1 << (s - 1))) >> s
 *                columns first with s = 11, then rows with s = 18, then clamp(x + 128, 0, 255).  (libjpeg indexes a 1024-entry
 *                table with the low 10 bits instead of clamping, and its SIMD forms saturate earlier: values no 8-bit image
 *                encodes to.  The clamp is what is built; PIL's bytes are pinned for real files, tests/golden/jpeg_pil.npz.)
 *   crop         each chroma plane to cw x ch = ceil(width / hs) x ceil(height / vs) before upsampling: neighbours clamp there
 *   2 x 1        out[2c] = (3 in[c] + in[c-1] + 1) >> 2; out[2c+1] = (3 in[c] + in[c+1] + 2) >> 2; a missing neighbour is in[c]
 *   2 x 2        cs[c] = 3 row[r][c] + row[r-1 for an even output row, r+1 for an odd one, clamped to the plane][c]
 *                out[2c] = (3 cs[c] + cs[c-1] + 8) >> 4; out[2c+1] = (3 cs[c] + cs[c+1] + 7) >> 4; a missing neighbour is cs[c]
 *   cw <= 2      libjpeg takes its replicating upsamplers: out[y][x] = in[y / vs][x / 2]
 *   colour       cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16); B = Y + ((116130 cb + 32768) >> 16);
 *                G = Y + ((-22554 cb - 46802 cr + 32768) >> 16); each clamped to 0 .. 255
 * No allocation, no host synchronisation, no atomics; the result does not depend on the launch shape.
 * GA_ERR_BAD_ARG, nothing launched -- from ga_jpeg_check_table on a HOST copy of the table before it is staged: a row that is not one
 * of the forms above or whose MCU grid is not the one that covers the image; coefficients, tables, planes or image outside their
 * buffers (coef_count and qt_count in elements) or off the 16-byte grid -- and from ga_jpeg_reconstruct: a null or misaligned pointer,
 * n_images outside 1 .. 65535.  The kernels clamp nothing: a table that fails the check must never reach them. */
int ga_jpeg_probe(const uint8_t* bytes, size_t n, int64_t* info);
int ga_jpeg_entropy_decode(const uint8_t* bytes, size_t n, int16_t* coef, size_t coef_capacity, uint16_t* qt);
int ga_jpeg_check_table(const void* rows_host, int n_images, uint64_t coef_count, uint64_t qt_count, uint64_t work_bytes,
                        uint64_t dst_bytes);
size_t ga_jpeg_work_bytes(const void* rows_host, int n_images);
int ga_jpeg_reconstruct(const void* table, int n_images, const int16_t* coef, const uint16_t* qt, void* work, void* dst,
                        ga_stream_t stream);
/* adaptive gradient clipping (timm adaptive_clip_grad, clip_mode 'agc'): units = int64 {offset, length} pairs into the flat fp32
 * parameter / gradient buffers (a row of a >= 2-d parameter or a whole <= 1-d one); per unit
 * g *= max(|p|, eps) * clip_factor / max(|g|, 1e-6) where |g| exceeds max(|p|, eps) * clip_factor */
int ga_agc_clip(const float* params, float* grads, const int64_t* units, int nunits, float clip_factor, float eps, ga_stream_t stream);
int ga_gelu_fwd(const void* x, void* y, int64_t n, int dtype, ga_stream_t stream);
int ga_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, ga_stream_t stream);
int ga_relu_drop(const void* a, const float* mask, void* out, void* deriv, int64_t n, int dtype, ga_stream_t stream);
int ga_mask_mul(const void* x, const float* mask, const void* res, void* y, int64_t n, int dtype, ga_stream_t stream);
int ga_copy2d(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int cols, int accumulate, int dtype,
              ga_stream_t stream);

/* DropPath masks of a training step (timm DropPath: ga_convnext.py:96,111; ga_cswin.py:181,209-210):
 *   out[s][b] = Bernoulli(keep[s]) / keep[s]  for `sites` stochastic-depth sites x B samples, from a counter-based
 *   generator keyed by (seed, *counter, element); *counter (device memory) is advanced by one per call. */
int ga_drop_path_sample(float* out, const float* keep, int sites, int B, uint64_t seed, uint64_t* counter, ga_stream_t stream);

/* nn.Dropout masks of the MAP head (map.py:54,82-83): out[i] = Bernoulli(keep) / keep, i < n; *counter advanced by one */
int ga_dropout_mask_sample(float* out, int64_t n, float keep, uint64_t seed, uint64_t* counter, ga_stream_t stream);

/* Fused MLP bodies of the narrow stages (bf16, C in {96, 192}, H = 4C; ga_mlp_supported tells): the [M][H] hidden activation
 * stays on chip.  Replaces the fc1 / fc2 pair of ga_gemm launches of a ConvNeXt Block (ga_convnext.py:86-101) and, backward,
 * the dgrad2 / dgrad1 pair:
 *   ga_mlp_fwd: Y = R + rowscale[m / rows_per_scale] * (gelu(X W1^T + b1) W2^T + b2)      (R, rowscale optional)
 *               W1 [H][ldw1] (rows = hidden), W2 [C][ldw2] (rows = output channel): the effective weights of ga_weight_prep;
 *   ga_mlp_bwd: Hd = X W1^T + b1 re-computed;  A = gelu(Hd) -> A [M][lda];  DH = (DY W2) * gelu'(Hd) -> DH [M][lddh];
 *               DX = DH W1 -> DX [M][lddx].  W2T [H][ldw2t] = W2 transposed (rows = hidden), W1T [C][ldw1t] = W1 transposed.
 *               The two weight-gradient GEMMs (ga_wgrad) then read A / DH exactly as they read the stored tensors before.
 * GELU is the tanh form the bf16 fc1 epilogue of ga_gemm uses (|error| <= 5e-4, below the bf16 rounding of the result). */
typedef struct {
    const void* X; int64_t ldx;
    const void* W1; int64_t ldw1; const float* b1;
    const void* W2; int64_t ldw2; const float* b2;
    const void* R; int64_t ldr;
    const float* rowscale; int rows_per_scale;
    void* Y; int64_t ldy;
    int64_t M; int C, H, dtype;
} ga_mlp_desc;
typedef struct {
    const void* X; int64_t ldx;
    const void* DY; int64_t lddy;
    const void* W1; int64_t ldw1; const float* b1;
    const void* W2T; int64_t ldw2t;
    const void* W1T; int64_t ldw1t;
    void* A; int64_t lda;
    void* DH; int64_t lddh;
    void* DX; int64_t lddx;
    int64_t M; int C, H, dtype;
    /* optional (all zero: the launch above).  dW1 given: the fc1 weight gradient is accumulated inside the kernel, from the DH
     * and X tiles it holds on chip, so DH need not be stored for a ga_wgrad launch:
     *   dW1 [H][ldw] fp32 += DH^T X,  db1 [H] fp32 += column sums of DH   (DH as rounded to bf16, fp32 accumulation)
     * C = 96 only (ga_mlp_bwd_wgrad_supported; an error otherwise).  The launch is then persistent: each workgroup walks
     * several 128-row tiles and leaves one fp32 partial [H*C + H] in `partials` (caller-owned scratch of ga_mlp_bwd_partials(d)
     * bytes, 16-byte aligned, dead once the call's work is done); a second kernel adds the partials in a fixed order -- no
     * float atomics, two runs give the same bits.  max_blocks: 0 = as many workgroups as are resident at once, else a cap. */
    float* dW1; int64_t ldw;
    float* db1;
    float* partials; size_t partials_bytes;
    int max_blocks;
} ga_mlp_bwd_desc;
int ga_mlp_supported(int C, int H, int dtype);
int ga_mlp_fwd(const ga_mlp_desc* d, ga_stream_t stream);
/* A / DH may each be NULL: that tensor is not stored */
int ga_mlp_bwd(const ga_mlp_bwd_desc* d, ga_stream_t stream);
int ga_mlp_bwd_wgrad_supported(int C, int H, int dtype);
/* bytes of `partials` the descriptor's launch with dW1 needs (depends on M, max_blocks and the device; the pointers are not
 * looked at); 0 where ga_mlp_bwd_wgrad_supported says no */
size_t ga_mlp_bwd_partials(const ga_mlp_bwd_desc* d);

/* Alignment-free forms for the odd-width variants (ga_convnext_*_688, base_976: 86 / 172 / 122 / 244 channels per group are off
 * the 16-byte grid of the MFMA kernels).  The heads' grouped 1x1 convolutions act on one token per image (rows = batch):
 *   ga_small_linear_fwd: Y[r][g*Ng + n] = R + rowscale[r / rps] * col_scale[.] * (sum_k A[r][col(g*a_gstride + k)] W[g*Ng + n][k] + bias[.])
 *     A / Y / R / Yraw in `dtype`, element-wise loads (any alignment); W [groups*Ng][Kg], bias, col_scale: the fp32 MASTER
 *     parameters, no weight preparation; col(c) = a_perm ? a_perm[c] : c (the channel_shuffle of GroupConvMlp, ga_convnext.py:557-566);
 *     Yraw (optional, leading dimension ldy) keeps the value before col_scale for the col_scale gradient.
 *   ga_small_linear_bwd (same descriptor): dA (+)= dYeff W;  dW += dYeff^T A;  dbias += colsum(dYeff);  dcol_scale += colsum(dY * rowscale * Yraw)
 *     with dYeff = dY * rowscale * col_scale; any of dA / dW / dbias / dcol_scale may be NULL.
 *   ga_colstats: sum[c] += sum_r x[r][c], sumsq[c] += sum_r x^2 (the BatchNorm batch statistics ga_gemm's epilogue otherwise delivers).
 *   ga_pad_copy_f32: dst[r][0..cols) (+)= src[r][0..cols), row strides lds / ldd in elements: parameters of the 172 / 244-wide stage-4
 *     Bottleneck into zero-padded 176 / 248-wide buffers for the MFMA kernels, and their gradients back. */
typedef struct {
    int rows, groups, Ng, Kg;
    const void* A; int64_t lda; int64_t a_gstride; const int* a_perm;
    const float* W; const float* bias; const float* col_scale;
    const float* rowscale; int rows_per_scale;
    const void* R; int64_t ldr;
    void* Y; int64_t ldy; void* Yraw;
    int dtype;
} ga_small_linear_desc;
int ga_small_linear_fwd(const ga_small_linear_desc* d, ga_stream_t stream);
int ga_small_linear_bwd(const ga_small_linear_desc* d, const void* dY, void* dA, int accumulate_dA, float* dW, float* dbias,
                        float* dcol_scale, ga_stream_t stream);
int ga_colstats(const void* x, int64_t ld, int rows, int C, float* sum, float* sumsq, int dtype, ga_stream_t stream);
int ga_pad_copy_f32(const float* src, float* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd, int accumulate, ga_stream_t stream);
/* ConvNeXt stem in one pass (timm ConvNeXt stem / ga_convnext.py:431-434: Conv2d(3, C, 4, 4) + LayerNorm over the channels), bf16:
 *   x fp32 NCHW [B][3][H][W];  W bf16 [C][ldw], k = (c, ky, kx) as ga_weight_prep(stem = 1) writes it;  bias / gamma / beta fp32 [C];
 *   pre [B*H/4*W/4][C] = conv + bias (kept for ga_layernorm_bwd), y = LayerNorm(pre) * gamma + beta, mean / rstd per pixel.
 *   Equals ga_gemm(GA_A_STEM4_NCHW, bias) followed by ga_layernorm_fwd on the rounded `pre`.  C = 96 or 128. */
int ga_stem4_ln_fwd(const float* x, const void* W, int64_t ldw, const float* bias, const float* gamma, const float* beta, void* pre,
                    void* y, float* mean, float* rstd, int B, int H, int W_, int C, float eps, ga_stream_t stream);
/* grouped 1x1 convolution as ONE dense GEMM: the weight [R][cg] of a conv with ng groups (rg output rows and cg input channels per
 * group; R = a multiple of rg * ng: several such weights stacked) <-> its block-diagonal image [R][ld] (row r's values at columns
 * ((r / rg) % ng) * cg ..., zeros elsewhere, zero-initialised by the caller).  to_diag = 1 writes the block-diagonal side, 0 reads it back ((+)= with accumulate).  GA-CSWin's grouped gram_contraction
 * (ga_cswin.py:559-561: 8 groups of 64 -> 24 channels, five heads) runs as one 960 x 512 product instead of 40 products with N = 24. */
int ga_blockdiag_f32(const float* src, float* dst, int64_t R, int rg, int ng, int cg, int64_t ld, int to_diag, int accumulate,
                     ga_stream_t stream);
/* two-level group padding of an fp32 parameter matrix [R][C] <-> [R/RG*RGp][C/CG*CGp] (rows in groups of RG padded to RGp, columns
 * in groups of CG padded to CGp; the padded side is zero-initialised by the caller): unpad = 0 writes the padded matrix, unpad = 1
 * reads it back ((+)= with accumulate).  The grouped one-token layers of the odd-width variants (GroupConvMlp of ga_convnext_*_688 /
 * base_976, ga_convnext.py:190-222: 172 / 244 channels per group) run on the MFMA kernels over such copies. */
int ga_pad_groups_f32(const float* src, float* dst, int64_t R, int64_t C, int RG, int RGp, int CG, int CGp, int unpad, int accumulate,
                      ga_stream_t stream);
/* the same element-wise strided copy for activations in `dtype` (group compaction: [rows*groups][88] -> [rows*groups][86]) */
int ga_pad_copy(const void* src, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd, int accumulate, int dtype,
                ga_stream_t stream);

/* Global multi-head self-attention (timm vision_transformer.Attention inside `Block`, MAP/models/map_pit.py:14,35-44):
 *   qkv [B*N][ldq]: q | k | v column blocks of width C = H*hd (head h = columns h*hd.. of each block); out [B*N][ldo];
 *   out = softmax(q k^T * scale) v per (image, head);  lse [B][H][N] fp32 = row log-sum-exp, kept for the backward pass.
 * bf16 with hd in {16, 32, 48, 64} runs flash-style on MFMA (64-query workgroups, 64-key blocks streamed through LDS, online softmax);
 * everything else (fp32 parity mode, other hd <= 128) on a plain fp32 form meant for small batches.
 * bwd: dqkv [B*N][ldq] = d(q | k | v) from dout [B*N][ldo]; needs `out` and `lse` of the forward pass and a caller-owned
 * workspace of ga_attn_bwd_workspace(d) bytes (delta[b][h][q] = dout . out). */
typedef struct {
    int B, N, H, hd;
    float scale;
    int dtype;
    const void* qkv; int64_t ldq;
    void* out; int64_t ldo;
    float* lse;
} ga_attn_desc;
int ga_attn_fwd(const ga_attn_desc* d, ga_stream_t stream);
size_t ga_attn_bwd_workspace(const ga_attn_desc* d);
int ga_attn_bwd(const ga_attn_desc* d, const void* dout, void* dqkv, void* workspace, size_t ws_bytes, ga_stream_t stream);
/* ViT stem (timm PatchEmbed + cls_token / pos_embed; the P x P stride-P patch convolution becomes a ga_gemm over patches):
 *   ga_patchify:      fp32 NCHW [B,CH,H,W] -> [B*(H/P)*(W/P)][CH*P*P] in `dtype`, k = (c, ky, kx) (the conv weight's flattened order)
 *   ga_vit_embed_fwd: x0[b][0] = cls + pos[0];  x0[b][1+p] = tok[b][p] + pos[1+p]      (cls [C], pos [Np+1][C] fp32)
 *   ga_vit_embed_bwd: dtok = dx0[b][1+p];  dcls += sum_b dx0[b][0];  dpos[t] += sum_b dx0[b][t] */
int ga_patchify(const float* x, void* out, int B, int CH, int H, int W, int P, int dtype, ga_stream_t stream);
int ga_vit_embed_fwd(const void* tok, const float* cls, const float* pos, void* x0, int B, int Np, int C, int dtype, ga_stream_t stream);
int ga_vit_embed_bwd(const void* dx0, void* dtok, float* dcls, float* dpos, int B, int Np, int C, int dtype, ga_stream_t stream);

/* Pooling transformer (PiT) pieces around the ViT blocks -- /root/reference/MAP/models/map_pit.py
 *   ga_patchify_strided: conv_embedding (:71-81) as im2col for a patch convolution whose stride S differs from the patch size P
 *                        (16 / 8 in map_pit_s: overlapping patches): [B*gh*gw][CH*P*P], gh = (H - P) / S + 1; P % 8 == 0, S % 4 == 0
 *   ga_pos_add_fwd/bwd:  x0[b][p] = tok[b][p] + pos[p]  (:190-191; pos fp32 [Np][C], the NCHW parameter transposed);
 *                        dpos[p] = sum_b dx0[b][p]  (overwrites)
 *   ga_dwpool_*:         conv_head_pooling (:58-68): depthwise 3 x 3 / stride 2 / pad 1 convolution with a channel multiplier
 *                        (groups = Cin, Cout = mult * Cin) on NHWC maps [B][H][W][Cin] -> [B][Ho][Wo][Cout], Ho = (H - 1) / 2 + 1;
 *                        w fp32 [Cout][9] (the (Cout, 1, 3, 3) parameter), bias fp32 [Cout].  bwd_weight ACCUMULATES into dw / db.
 *   ga_resize_concat_*:  bilinear resize (align_corners = False, no antialias; any Hin x Win -> Hout x Wout) of an NHWC map into
 *                        columns [c_off, c_off + C) of the MultiScale concat buffer (row stride ldd); map.py:322-333 reduces
 *                        PiT's 27 x 27 maps to 14 x 14 this way.  bwd writes dsrc (gather form, no atomics). */
int ga_patchify_strided(const float* x, void* out, int B, int CH, int H, int W, int P, int S, int dtype, ga_stream_t stream);
int ga_pos_add_fwd(const void* tok, const float* pos, void* x0, int B, int Np, int C, int dtype, ga_stream_t stream);
int ga_pos_add_bwd(const void* dx0, float* dpos, int B, int Np, int C, int dtype, ga_stream_t stream);
int ga_dwpool_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int Cin, int mult, int dtype,
                  ga_stream_t stream);
int ga_dwpool_bwd_data(const void* dy, const float* w, void* dx, int B, int H, int W, int Cin, int mult, int dtype, ga_stream_t stream);
int ga_dwpool_bwd_weight(const void* dy, const void* x, float* dw, float* db, int B, int H, int W, int Cin, int mult, int dtype,
                         ga_stream_t stream);
int ga_resize_concat_fwd(const void* src, void* dst, int B, int Hin, int Win, int C, int Hout, int Wout, int64_t ldd, int c_off,
                         int dtype, ga_stream_t stream);
int ga_resize_concat_bwd(const void* dcat, void* dsrc, int B, int Hin, int Win, int C, int Hout, int Wout, int64_t ldd, int c_off,
                         int dtype, ga_stream_t stream);
/* dst[b][p][:] = scale * src[b][:], p < HW: the gradient of the global average pool of the plain ConvNeXt head
 * (MAP/models/map_convnext.py:134-135, `x.mean([-2, -1])`; scale = 1 / HW) */
int ga_rows_bcast(const void* src, void* dst, int B, int HW, int C, float scale, int dtype, ga_stream_t stream);
/* global average pool over the tokens of a [B][N][C] sequence: the pool_type='gap' head of the plain PiT
 * (MAP/models/map_pit.py:194, `x[-1].mean([-2, -1])`).  x, y, dy, dx are of the activation dtype.
 *   ga_token_gap_fwd: y[b][c] = (1/N) * sum_n x[b][n][c]; fp32 accumulation in a fixed order, no atomics: bitwise repeatable
 *   ga_token_gap_bwd: dx[b][n][c] = dy[b][c] / N (overwrites dx): a correctly rounded fp32 quotient, then the rounding of the store
 * 16-byte loads and stores when C is a multiple of 8 (bf16) / 4 (fp32) and the pointers are 16-byte aligned; any other C or
 * alignment runs the one-element form of the same kernels.  N <= 2^24. */
int ga_token_gap_fwd(const void* x, void* y, int B, int N, int C, int dtype, ga_stream_t stream);
int ga_token_gap_bwd(const void* dy, void* dx, int B, int N, int C, int dtype, ga_stream_t stream);

/* small fp32 / elementwise utilities */
int ga_memset(void* p, int value, size_t bytes, ga_stream_t stream); /* hipMemsetAsync on `stream` */
int ga_transpose_f32(const float* in, float* out, int R, int C, int accumulate, ga_stream_t stream); /* out[c][r] (+)= in[r][c] */
int ga_axpy_f32(float* y, const float* x, float a, int64_t n, ga_stream_t stream);
int ga_lerp_f32(float* y, const float* x, float w, int64_t n, ga_stream_t stream); /* y += w*(x-y): ModelEmaV2 update, GA/train.py:499 */
int ga_rowscale(const void* x, const float* s, void* y, int64_t n, int64_t elems_per_scale, int dtype,
                ga_stream_t stream);
int ga_cast_from_f32(const float* src, void* dst, int64_t n, int dtype, ga_stream_t stream);
int ga_cast_to_f32(const void* src, float* dst, int64_t n, int dtype, ga_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient exchange over RCCL / xGMI.  replaces: NativeDDP(model, device_ids=[local_rank]) and its bucket reducer
 * (GA/train.py:514, MAP/train.py:576), the per-forward buffer broadcast (`broadcast_buffers`), timm distribute_bn
 * (GA/train.py:665-674).  One communicator per process (one process per GPU).  The 128-byte id comes from rank 0
 * (ga_comm_unique_id) and reaches the other ranks through the caller's side channel (torch.distributed's store in
 * imagenet_models_amd.comm).  librccl is resolved at run time: GA_ERR_UNSUPPORTED when it cannot be loaded.
 * Every call only enqueues on `stream`; buffers are caller-owned device memory.
 *   ga_allreduce_bucket:      grads[0..n) := scale * sum over ranks, in place.  wire_dtype GA_F32: ncclAllReduce on the slice;
 *                             GA_BF16: packed to bf16 in `workspace` (ga_allreduce_workspace(n, GA_BF16) bytes), reduced in
 *                             bf16, unpacked -- half the wire bytes, bf16 summation (an option, not the default).
 *   ga_reduce_scatter_bucket: shard[0..n_per_rank) := scale * sum over ranks of grads[rank*n_per_rank ..] (grads holds
 *                             world * n_per_rank elements); ga_allgather_bucket is its inverse.  Together they are the
 *                             all-reduce with room for a sharded (ZeRO-1) optimizer step in between.
 *   ga_comm_broadcast:        n_f32 floats from `root` (initial parameters, BatchNorm running statistics).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct ga_comm* ga_comm_t;
int ga_comm_unique_id(void* id128);
int ga_comm_init(ga_comm_t* comm, int rank, int world, const void* id128);
int ga_comm_destroy(ga_comm_t comm);
int ga_comm_info(ga_comm_t comm, int* rank, int* world);
size_t ga_allreduce_workspace(int64_t n, int wire_dtype);
int ga_allreduce_bucket(ga_comm_t comm, float* grads, int64_t n, int wire_dtype, float scale, void* workspace, size_t ws_bytes,
                        ga_stream_t stream);
int ga_reduce_scatter_bucket(ga_comm_t comm, const float* grads, float* shard, int64_t n_per_rank, float scale, ga_stream_t stream);
int ga_allgather_bucket(ga_comm_t comm, const float* shard, float* full, int64_t n_per_rank, ga_stream_t stream);
int ga_comm_broadcast(ga_comm_t comm, void* buf, int64_t n_f32, int root, ga_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GAEXT_H */
