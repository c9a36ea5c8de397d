/*
 * hcunet.h -- C-ABI of the MI355X-native 3D U-Net training hot path.
 *
 * This library replaces the arithmetic behind the reference's Python operator
 * interface for ONE path: hcat.unet.Unet_Constructor forward + backward, the
 * pixel-weighted BCE loss (hcat.loss.cross_entropy, method='pixel') and the
 * Adam step that follows it in the reference training pattern -- plus the
 * callers either side of it: the tiled inference driver, the
 * input transforms and the reference's other losses.  The reference
 * binds no native code (it calls stock torch.nn ops), so each entry point below
 * names the reference symbol whose semantics it implements; the Python host
 * layer (hcunet_amd/, re-exported as hcat.unet / hcat.loss) binds these through
 * ctypes.
 *
 * Conventions
 *   - Every pointer is a device (HBM) pointer owned by the caller.  No entry
 *     point allocates device memory for tensors; scratch/saved workspaces are
 *     sized by the *_bytes / *_query functions and passed in.  One exception:
 *     creating a TRAINING plan times the best few convolution tilings on a
 *     private, grown-on-demand device arena (hipMalloc, kept for the process;
 *     HCU_BCONV_TUNE=0 disables the timing).
 *   - Work is enqueued asynchronously on `stream` (a hipStream_t, 0 = null
 *     stream).  The per-op launchers are stateless and re-entrant.
 *   - A network plan (hcu_unet_plan) is NOT read-only after creation: on first
 *     use it lazily creates, on the calling thread's current device, a private
 *     capture stream and up to 8 instantiated hipGraphs per distinct set of
 *     buffer pointers (guarded by a mutex), and for the backward a private
 *     weight-gradient stream plus fork/join/slot events.  The backward enqueues
 *     its weight-gradient branch on that private stream, ordered against the
 *     caller's stream by events (fork after the caller's prior work, join before
 *     the call returns its work to the caller's stream), so callers observe
 *     ordinary stream order.  Concurrent backwards of one plan serialise on the
 *     plan's mutex.  Call with the device of the tensors current (the Python
 *     layer does).  A failed capture destroys the branch stream; it is
 *     recreated on the next backward.
 *   - Return value: HCU_OK or an error code; no C++ exception crosses the ABI.
 *     hcu_last_error() returns a thread-local message for the last failure.
 *   - Activation tensors handled by the per-op entry points are channels-last
 *     fp32: [B][X][Y][Z][Cs] with Cs = round_up(C, 4).  The network entry points
 *     take the reference's NCXYZ ([B][C][X][Y][Z], PyTorch NCDHW) tensors.
 *   - Weight tensors are always in PyTorch layout: Conv3d [Cout][Cin/g][kx][ky][kz],
 *     ConvTranspose3d [Cin][Cout][kx][ky][kz].
 */
#ifndef HCUNET_H
#define HCUNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *hcu_stream_t; /* hipStream_t */

enum {
  HCU_OK = 0,
  HCU_ERR_INVALID = 1,     /* bad argument (maps to ValueError / TypeError) */
  HCU_ERR_SHAPE = 2,       /* shape error   (maps to RuntimeError, as torch raises) */
  HCU_ERR_HIP = 3,         /* HIP runtime error */
  HCU_ERR_UNSUPPORTED = 4, /* configuration the reference itself rejects */
  HCU_ERR_WORKSPACE = 5    /* workspace too small */
};

enum { HCU_F32 = 0, HCU_F16 = 1, HCU_U8 = 2, HCU_BF16 = 3, HCU_U16 = 4, HCU_F64 = 5,
       HCU_I32 = 6, HCU_U32 = 7 /* label ids (training targets) */ };

const char *hcu_last_error(void);
int hcu_version(void);

/* ------------------------------------------------------------------------ */
/* Whole-network executor.                                                   */
/* Replaces: Unet_Constructor.__init__ shape logic  hcat/unet.py:16-123      */
/*           Unet_Constructor.forward               hcat/unet.py:125-143     */
/*           Down.forward / Up.forward / crop       hcat/unet.py:263-340     */
/*           and their autograd backward (torch.nn ops' derivatives).        */
/* ------------------------------------------------------------------------ */
#define HCU_MAX_LEVELS 12

typedef struct hcu_unet_spec {
  int levels;                       /* len(feature_sizes)                   */
  int in_channels, out_channels;
  int features[HCU_MAX_LEVELS];     /* feature_sizes                        */
  int k1[3], k2[3];                 /* kernel['conv1'], kernel['conv2']     */
  int d1[3], d2[3];                 /* dilation['conv1'], dilation['conv2'] */
  int g1, g2;                       /* groups['conv1'], groups['conv2']     */
  int up_k[3], up_s[3];             /* upsample_kernel, upsample_stride     */
  int pool_k[3];                    /* max_pool_kernel (kernel = stride)    */
  float bn_eps;                     /* BatchNorm3d eps (1e-5)               */
  float bn_momentum;                /* 0.1; < 0 means momentum=None         */
  int compute_dtype;                /* HCU_F32: fp32 throughout (the reference's
                                       arithmetic); HCU_BF16: bf16 activations,
                                       gradients and GEMM operands, fp32
                                       accumulation / statistics / parameters
                                       (torch.autocast(dtype=torch.bfloat16)) */
} hcu_unet_spec;

typedef struct hcu_unet_plan hcu_unet_plan;

/* Validates the spec against an input of [B, in_channels, X, Y, Z] and builds
 * the launch plan.  Fails with HCU_ERR_SHAPE where torch would raise (input
 * smaller than a kernel, pooled size 0, upsampled tensor larger than the skip
 * tensor so that torch.cat raises: hcat/unet.py:311-312). */
int hcu_unet_plan_create(const hcu_unet_spec *spec, int B, int X, int Y, int Z,
                         hcu_unet_plan **out);
void hcu_unet_plan_destroy(hcu_unet_plan *plan);

/* Plan flags.  HCU_PLAN_FORWARD_ONLY: inference (torch.no_grad) plan -- the
 * forward keeps no activation for a backward (they alternate between two
 * buffers of the largest activation), so saved_bytes is a small fraction of a
 * training plan's; hcu_unet_backward on it fails with HCU_ERR_INVALID.
 * Replaces the `with torch.no_grad(): unet(tile)` call of the reference's tiled
 * inference loop (hcat/segment.py:82-99), which keeps autograd off but still
 * runs the module's ordinary forward. */
#define HCU_PLAN_FORWARD_ONLY 1
int hcu_unet_plan_create_ex(const hcu_unet_spec *spec, int B, int X, int Y, int Z, int flags,
                            hcu_unet_plan **out);

/* out_shape[5] = output [B, out_channels, OX, OY, OZ]; n_params = number of
 * parameter scalars (flat layout = Unet_Constructor.parameters() order);
 * n_bn = number of BatchNorm3d modules; saved_bytes = forward->backward
 * workspace; scratch_bytes = per-call temporary workspace. */
int hcu_unet_plan_query(const hcu_unet_plan *plan, int64_t *out_shape,
                        int64_t *n_params, int *n_bn, size_t *saved_bytes,
                        size_t *scratch_bytes);

typedef struct hcu_unet_tensors {
  const float *x;          /* [B][Cin][X][Y][Z] of x_dtype (fp32 by default) */
  float *out;              /* [B][Cout][OX][OY][OZ] fp32                     */
  const float *params;     /* flat fp32, Unet_Constructor.parameters() order */
  float *grads;            /* flat fp32, same layout (backward only)         */
  float *const *bn_running_mean; /* n_bn pointers: down[i].batch1, batch2 ... */
  float *const *bn_running_var;  /*   then up[j].batch1, batch2 (module order) */
  int64_t *const *bn_num_batches_tracked;
  void *saved;             /* saved_bytes   */
  void *scratch;           /* scratch_bytes */
  int x_dtype;             /* HCU_F32, or with compute_dtype HCU_BF16 also
                              HCU_F16 / HCU_BF16 (16-bit volumes are read
                              directly by the channels-last staging kernel) */
} hcu_unet_tensors;

/* training != 0: BatchNorm uses batch statistics and updates running stats
 * (nn.BatchNorm3d train mode); 0: running statistics (eval mode). */
int hcu_unet_forward(const hcu_unet_plan *plan, const hcu_unet_tensors *t,
                     int training, hcu_stream_t stream);

/* dout: [B][Cout][OX][OY][OZ] gradient of the output.  Writes (accumulate=0)
 * or adds (accumulate=1) parameter gradients into t->grads; dx (nullable)
 * receives the input gradient [B][Cin][X][Y][Z].  Must follow a forward with
 * the same plan, tensors and training flag. */
int hcu_unet_backward(const hcu_unet_plan *plan, const hcu_unet_tensors *t,
                      const float *dout, float *dx, int training,
                      int accumulate, hcu_stream_t stream);

/* Introspection of the saved workspace (tests, debugging): one record per
 * BatchNorm3d in module order (down[i].batch1, batch2, ..., up[j].batch1,
 * batch2).  y_offset: byte offset in `saved` of that layer's pre-BatchNorm conv
 * output y, channels-last [B][X][Y][Z][Cs] of elem_bytes-sized elements;
 * coef_offset: byte offset of 6 fp32 arrays of Cs (scale, shift, mean, invstd,
 * c1, c0) with which the forward applied relu(y*scale + shift).  Returns the
 * number of records (written up to max). */
typedef struct hcu_bn_layer_info {
  int64_t y_offset, coef_offset;
  int B, X, Y, Z, C, Cs;
  int elem_bytes;
  int pad;
} hcu_bn_layer_info;
int hcu_unet_plan_bn_layers(const hcu_unet_plan *plan, hcu_bn_layer_info *out, int max);

/* ------------------------------------------------------------------------ */
/* Layer chains: a short sequence of Conv3d [+ BatchNorm3d + ReLU] /         */
/* MaxPool3d / ConvTranspose3d [+ cat(U, U)] ops run by the same kernels and */
/* fusions as the network executor, as one autograd node.  Replaces:         */
/*   Down.forward / Up.forward of hcat/unet.py:263-266, 309-315 called on    */
/*   their own, and the layers of hcat/r_unet.py: its Down / Up (padding,    */
/*   :249-336), f (:232-246), RDCNet's strided / 1x1 / padded ConvTranspose3d */
/*   (:207-227) and StackedDilation's dilated 5^3 convolutions (:339-364).   */
/* Input / output tensors are NCXYZ fp32 (the output with the last op's      */
/* BatchNorm + ReLU applied); parameters / gradients live in flat fp32       */
/* buffers at the per-op offsets; BatchNorm running statistics are passed    */
/* per BatchNorm op (hcu_unet_tensors' arrays, in op order).  Plans are      */
/* hcu_unet_plan objects (hcu_unet_plan_destroy frees them); a handle of the */
/* other kind is refused with HCU_ERR_INVALID by hcu_chain_* and hcu_unet_*  */
/* alike (hcu_unet_plan_query and hcu_unet_plan_destroy take both).          */
/* ------------------------------------------------------------------------ */
enum { HCU_CHAIN_CONV = 0, HCU_CHAIN_POOL = 1, HCU_CHAIN_CONVT = 2 };
#define HCU_CHAIN_MAX_OPS 16
typedef struct hcu_chain_op {
  int kind;                  /* HCU_CHAIN_*                                   */
  int out_channels;          /* CONV / CONVT                                  */
  int k[3], stride[3], dil[3], pad[3];   /* CONV; CONVT: k, stride, pad (crop) */
  int groups;                /* CONV                                          */
  int bn_relu;               /* CONV: followed by BatchNorm3d + ReLU          */
  int cat_fold;              /* CONV right after a CONVT: its input is cat(U, U)
                                (hcat/unet.py:311-312; the weight has 2*C input
                                channels per group and is folded)              */
  int64_t w_off, b_off;      /* float offsets of weight / bias (b_off < 0: none) */
  int64_t gamma_off, beta_off;   /* BatchNorm weight / bias (bn_relu)         */
} hcu_chain_op;
typedef struct hcu_chain_spec {
  int n_ops;
  int in_channels;
  hcu_chain_op ops[HCU_CHAIN_MAX_OPS];
  float bn_eps, bn_momentum;     /* < 0 momentum: cumulative average (None)   */
  int compute_dtype;             /* HCU_F32 or HCU_BF16 (as hcu_unet_spec)    */
  /* Channels-last boundaries (the recurrences of hcat/r_unet.py:219-225 keep
   * their state in the executor's layout between chains instead of NCXYZ):
   * in_cl / out_cl != 0: t->x / t->out (and dx / dout) are [B][X][Y][Z][Cs]
   * tensors of the compute dtype, Cs = the channel count rounded up to 8
   * (bf16) / 4 (fp32), padding channels zero.  in_part_channels > 0 (with
   * in_cl; the first op a Conv3d): the input is the channel-wise cat of
   * in_channels / in_part_channels such tensors, each padded on its own
   * (Cs = parts * round_up(in_part_channels)), i.e. torch.cat(..., dim=-1)
   * of channels-last chain outputs.  out_cl needs a last op that is a Conv3d
   * without BatchNorm. */
  int in_cl, out_cl, in_part_channels;
} hcu_chain_spec;
/* Fails with HCU_ERR_SHAPE where torch would raise for the input shape, with
 * HCU_ERR_UNSUPPORTED for op combinations the chain does not run (a MaxPool3d
 * not fed by Conv3d + BatchNorm3d + ReLU, a strided Conv3d's input gradient). */
int hcu_chain_plan_create(const hcu_chain_spec *spec, int B, int X, int Y, int Z,
                          hcu_unet_plan **out);
int hcu_chain_plan_query(const hcu_unet_plan *plan, int64_t *out_shape, int *n_bn,
                         size_t *saved_bytes, size_t *scratch_bytes);
/* t->x, t->out: NCXYZ fp32 (or channels-last, in_cl / out_cl); t->params /
 * t->grads: flat buffers of the op offsets; training as hcu_unet_forward. */
int hcu_chain_forward(const hcu_unet_plan *plan, const hcu_unet_tensors *t, int training,
                      hcu_stream_t stream);
int hcu_chain_backward(const hcu_unet_plan *plan, const hcu_unet_tensors *t, const float *dout,
                       float *dx, int training, int accumulate, hcu_stream_t stream);
/* The same with the packed weight images (the executor's re-layout of the
 * op weights, normally rebuilt in `saved` by every forward) kept in a
 * caller-owned buffer of hcu_chain_weight_image_bytes(plan) that outlives the
 * calls: a recurrence applying one chain several times per step re-lays them
 * once.  images_current: 0 = re-lay (the parameters changed since the images
 * were written), 1 = the buffer holds the forward images of the current
 * parameters (an eval forward wrote it), 2 = forward and input-gradient
 * images (a training forward wrote it).  The backward must be given the
 * buffer its forward used; after an eval-mode forward (images_current < 2)
 * it writes the input-gradient images into that buffer, so it is not const. */
size_t hcu_chain_weight_image_bytes(const hcu_unet_plan *plan);
int hcu_chain_forward_images(const hcu_unet_plan *plan, const hcu_unet_tensors *t, int training,
                             hcu_stream_t stream, void *images, int images_current);
int hcu_chain_backward_images(const hcu_unet_plan *plan, const hcu_unet_tensors *t,
                              const float *dout, float *dx, int training, int accumulate,
                              hcu_stream_t stream, void *images, int images_current);

/* The gated recurrence of RecursiveUnet.forward (hcat/r_unet.py:150-155), n
 * fp32 elements: h = tanh(hp), z = sigmoid(zp), out = h_prev*z + (-1*z*h);
 * h_prev == NULL means ones (the t == 0 state, :152-153).  The backward writes
 * d(hp), d(zp) and (nullable) d(h_prev) from d(out). */
int hcu_gate_fwd(const float *hp, const float *zp, const float *h_prev, float *out, int64_t n,
                 hcu_stream_t stream);
int hcu_gate_bwd(const float *hp, const float *zp, const float *h_prev, const float *dout, float *dhp,
                 float *dzp, float *dh_prev, int64_t n, hcu_stream_t stream);

/* Channel cat of channels-last tensors ([rows][C], C the padded channel
 * slots): split = 0 writes full[r] = parts[0][r] ++ parts[1][r] ++ ...,
 * split = 1 the reverse (the cat's backward: one contiguous gradient per
 * part).  1..8 parts, 16-byte aligned, part_row_bytes multiples of 16.
 * Replaces torch.cat(..., dim=1) on RDCNet's recurrence (hcat/r_unet.py:223
 * cat(x, y) and :362 the StackedDilation cat) and its autograd backward. */
int hcu_cl_cat(void *const *parts, const int *part_row_bytes, int nparts, void *full, int64_t rows,
               int split, hcu_stream_t stream);

/* RDCNet's residual state under bf16 autocast (hcat/r_unet.py:223-225):
 * out = float(m) + y (fp32) and out_c = its bf16 cast, n elements (a
 * multiple of 8; m, out_c bf16).  The backward writes dy = g32 + float(gc)
 * and dm = bf16(dy); g32 or gc may be NULL (no contribution). */
int hcu_resid_fwd(const void *m, const float *y, float *out, void *out_c, int64_t n, hcu_stream_t stream);
int hcu_resid_bwd(const float *g32, const void *gc, float *dy, void *dm, int64_t n, hcu_stream_t stream);

/* The channel cat + 1x1x1 Conv3d (no BatchNorm) of RDCNet's recurrence on
 * bf16 channels-last channel parts, without the cat: hcat/r_unet.py:223
 * cat(x, y) -> RDCBlock.conv (:372-374) and :362 the cat of the dilated
 * branches -> StackedDilation.out_conv (:354-364), with their autograd
 * backward.  parts[i]: [nvox][part_cs] bf16 with part_c real channels
 * (Cin = nparts * part_c, 1..8 parts, part_cs a multiple of 8, 16-byte
 * aligned); w: the PyTorch weight [Cout][Cin] fp32, b: [Cout] or NULL; out /
 * dout: [nvox][out_cs] bf16 (out_cs = Cout rounded up to 8, padding 0).
 * Backward: dparts (NULL: no input gradients) in the parts' layout; dw / db
 * (db nullable) overwritten or, accumulate != 0, added to; work: scratch of
 * hcu_pw_conv_work_floats(...) floats.  Channel counts: nparts * part_cs <= 96
 * slots, out_cs <= 32. */
int hcu_pw_conv_forward(const void *const *parts, int nparts, int part_c, int part_cs, const float *w,
                        const float *b, void *out, int64_t nvox, int Cout, int out_cs, hcu_stream_t stream);
size_t hcu_pw_conv_work_floats(int64_t nvox, int nparts, int part_cs, int Cout);
int hcu_pw_conv_backward(const void *const *parts, int nparts, int part_c, int part_cs, const float *w,
                         const void *dout, int Cout, int out_cs, void *const *dparts, float *dw, float *db,
                         int64_t nvox, float *work, size_t work_floats, int accumulate, hcu_stream_t stream);

/* out = parts[0] + parts[1] + ... (n elements, fp32 accumulation in input
 * order, one rounding; bf = 1: bf16 tensors, else fp32; NULL parts skipped;
 * at most 16).  The gradient of a tensor read by several chains (RDCNet:
 * hcat/r_unet.py:223-225,362), which autograd would sum pairwise. */
int hcu_sum_parts(const void *const *parts, int nparts, void *out, int64_t n, int bf, hcu_stream_t stream);

/* Data-parallel overlap (hcunet_amd/dist.py): with events set, every later  */
/* hcu_unet_backward on `plan` records ev_decoder on its weight-gradient     */
/* stream once the decoder's parameter gradients (up_steps, out_conv) are    */
/* final, and ev_deep once those of encoder levels >= deep_level are, so a   */
/* caller can reduce those gradient ranges while the rest of the backward    */
/* runs (hcu_stream_wait_event on its communication stream).  Each event    */
/* costs one extra batched weight-gradient finalize launch.  NULL events:    */
/* nothing recorded (the default).  The events stay owned by the caller.     */
int hcu_unet_set_grad_events(hcu_unet_plan *plan, void *ev_decoder, void *ev_deep, int deep_level);
/* 1 when hcu_unet_backward records those events (direct launches), 0 when  */
/* its backward is replayed from a captured graph (HCU_GRAPHS=1), where a    */
/* record would only be a capture dependency: reduce after the backward.     */
int hcu_unet_grad_events_live(const hcu_unet_plan *plan);
int hcu_event_create(void **ev);          /* hipEventDisableTiming */
int hcu_event_destroy(void *ev);
int hcu_stream_wait_event(hcu_stream_t stream, void *ev);

/* Data parallel (hcunet_amd/dist.py): n <= 128 fp32 vectors (the BatchNorm
 * running statistics) gathered into (unpack = 0) or scattered from
 * (unpack = 1) one contiguous buffer in one launch, in order. */
int hcu_gather_vectors(float *const *vecs, const int *lens, int n, float *buf, int unpack,
                       hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Loss.  Replaces hcat.loss.cross_entropy(pred, mask, pwl, method='pixel')  */
/* hcat/loss.py:5-101: crop mask/pwl top-left to pred (:51-53), BCE with     */
/* logits * (pwl + 1) computed in pwl's dtype (:65,71-72), mean (:101).      */
/* pwl == NULL means weight 2 everywhere (:46-47).                            */
/* ------------------------------------------------------------------------ */
size_t hcu_loss_pixel_scratch_bytes(int64_t n_pred);
/* pred [B][C][PX][PY][PZ] fp32; mask/pwl [B][C][MX][MY][MZ] of dtype
 * mask_dtype / pwl_dtype (HCU_F32, HCU_F16, HCU_U8).  loss[0] <- mean loss;
 * dpred <- d(loss)/d(pred) for an upstream gradient of 1 (nullable). */
int hcu_loss_pixel_fwd(const float *pred, int B, int C, int PX, int PY, int PZ,
                       const void *mask, int mask_dtype, const void *pwl,
                       int pwl_dtype, int MX, int MY, int MZ, float *loss,
                       float *dpred, void *scratch, size_t scratch_bytes,
                       hcu_stream_t stream);
/* dst[i] = src[i] * scale[0] (scale is a device scalar: the upstream grad). */
int hcu_scale_by_device_scalar(const float *src, const float *scale, float *dst,
                               int64_t n, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* The reference's other losses (hcat/loss.py:5-178), same geometry as     */
/* hcu_loss_pixel_fwd.  mode: 0 cross_entropy(method='sigmoid') (:38-40,     */
/* :95-97), 1 method='worst_z' (:74-80), 2 dice (:104-126), 3 L1Loss         */
/* (:128-152), 4 MSELoss (:154-178), 5 plain BCE mean ('random' with no      */
/* positive pixel, :84-85), 6 'random' (hcu_loss_random_fwd, :86-93).        */
/* Forward writes loss[0] and aux (the scalars the gradient needs: 1 float,  */
/* 2 for dice, PZ for worst_z); backward writes dpred = dloss/dpred *        */
/* grad_out[0].  zscale (worst_z): torch.linspace(1, 2, PZ) ** 2 (:76).      */
/* ------------------------------------------------------------------------ */
size_t hcu_loss_ext_scratch_bytes(int mode, int64_t n_pred, int PZ);
int hcu_loss_ext_fwd(int mode, const float *pred, int B, int C, int PX, int PY, int PZ,
                     const void *mask, int mask_dtype, const void *pwl, int pwl_dtype,
                     int MX, int MY, int MZ, const float *zscale, float *loss, float *aux,
                     void *scratch, size_t scratch_bytes, hcu_stream_t stream);
int hcu_loss_ext_bwd(int mode, const float *pred, int B, int C, int PX, int PY, int PZ,
                     const void *mask, int mask_dtype, const void *pwl, int pwl_dtype,
                     int MX, int MY, int MZ, const float *aux, const int *counts,
                     const float *grad_out, float *dpred, hcu_stream_t stream);
/* 'random' (hcat/loss.py:82-93): rows = hcu_loss_random_rows(n);
 * hcu_loss_random_count writes counts[rows][2] = (#mask==1, #mask==0) per row
 * of the flattened cropped mask; the caller draws pos_ind / neg_ind (int64,
 * n each) from its generator as the reference does and passes the exclusive
 * row offsets; hcu_loss_random_fwd compacts the pixel lists (pos_list /
 * neg_list: #mask==1 / #mask==0 ints), gathers the 2n drawn pixels, writes
 * the mean BCE and adds each drawn pixel's draw count into counts_px
 * (n_pred ints, zeroed by the caller) for hcu_loss_ext_bwd(mode 6). */
int hcu_loss_random_rows(int64_t n_pred);
int hcu_loss_random_count(const float *pred, int B, int C, int PX, int PY, int PZ,
                          const void *mask, int mask_dtype, int MX, int MY, int MZ,
                          int *counts, hcu_stream_t stream);
int hcu_loss_random_fwd(const float *pred, int B, int C, int PX, int PY, int PZ,
                        const void *mask, int mask_dtype, int MX, int MY, int MZ,
                        const int *offsets, int *pos_list, int *neg_list,
                        const int64_t *pos_ind, const int64_t *neg_ind, int n,
                        int *counts_px, float *loss, float *aux, void *scratch,
                        size_t scratch_bytes, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Input path.  Replaces, for B raw volumes at once, the     */
/* reference's to_float (hcat/transforms.py:94-116) -> reshape (:139-157)    */
/* -> normalize (:257-283) -> to_tensor (:118-137) chain: src [B][Z][Y][X][C] */
/* of src_dtype HCU_U16 / HCU_U8 / HCU_F64; to_float: scale by 2^-16 / 2^-8; */
/* reshape: output [B][C][X][Y][Z] (else [B][C][Z][Y][X]); mean/std (host    */
/* arrays of C doubles, nullable): (v + -mean) / std.  Arithmetic in float64, */
/* one round-to-nearest-even to fp16: bit-identical to the reference.  dst:  */
/* fp16.  Fails with HCU_ERR_INVALID for other dtypes (the reference's       */
/* TypeError, :113-114).                                                      */
/* ------------------------------------------------------------------------ */
int hcu_ingest_volume(const void *src, int src_dtype, int B, int Z, int Y, int X, int C,
                      int to_float, int reshape, const double *mean, const double *std,
                      void *dst, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Input path with crops and augmentation: n_jobs independent volumes in ONE */
/* launch (the image, mask and pixel-weight map of every item of a batch).   */
/* A job reads a window of a raw stack src [Z][Y][X][C] (HCU_U16 / HCU_U8)   */
/* and writes the network input dst [n_chan][ox][oy][oz] fp16, i.e. the      */
/* reference's to_float (hcat/transforms.py:94-116) -> reshape (:139-157) -> */
/* crops -> per-voxel steps -> to_tensor (:118-137) chain:                   */
/*   window   output (i, j, k) reads source x = xmap ? xmap[i] : x0 + i,     */
/*            y = ymap ? ymap[j] : y0 + j, z = z0 + k: random_crop's window  */
/*            (:337-396) composed with nul_crop's keep lists (:460-489);     */
/*   channels output channel c reads source channel chan[c]                  */
/*            (remove_channel, :590-613);                                    */
/*   steps    v = src * scale, then the program in recorded order, float64,  */
/*            a / b the operands of output channel c:                        */
/*     HCU_AUG_NORMALIZE  v = (v + -a) / b                  normalize :257-283 */
/*     HCU_AUG_INTENSITY  v -= a; v<0 -> 0, NaN -> 0, Inf -> 1              */
/*                                                   random_intensity :301-334 */
/*     HCU_AUG_DROP       a != 0: v = 0                  drop_channel :285-298 */
/*     HCU_AUG_CLEAN      NaN -> 0, +-Inf -> 1            clean_image :616-631 */
/*     HCU_AUG_GAMMA      v = pow(v, a), v >= 0          random_gamma :186-197 */
/*     HCU_AUG_SPEKLE     v += (float)(a * n), then v<0 -> 0, v>1 -> 1, n a   */
/*                        standard normal (Philox-4x32-10 keyed by key, the   */
/*                        job and step index, the output voxel and the channel */
/*                        pair; Box-Muller in float64, cosine branch for the   */
/*                        even channel, sine for the odd): the distribution of */
/*                        spekle (:159-183), not numpy's stream;               */
/*   rotation (rot = 1) random_rotate (:230-254): scipy.ndimage.rotate in the  */
/*            (x, y) plane, order 0, zeros outside.  The window above then     */
/*            describes the PRE-rotation view of rot_nx by rot_ny voxels (maps */
/*            of rot_nx / rot_ny entries) and output (i, j, k) is voxel        */
/*            (u, v) = (rot_px + i, rot_py + j) of the rotated view, whose     */
/*            source is, in float64 with every product and sum rounded on its  */
/*            own (no fused multiply-add),                                     */
/*              cx = (u * rot_m[0] + v * rot_m[1]) + rot_off[0]                */
/*              cy = (u * rot_m[2] + v * rot_m[3]) + rot_off[1]                */
/*            view voxel (floor(cx + 0.5), floor(cy + 0.5)) when               */
/*            0 <= cx <= rot_nx - 1 and 0 <= cy <= rot_ny - 1, and otherwise   */
/*            the constant 0.0 AS OF STEP fill_after: steps [0, fill_after)    */
/*            act on the gathered source value only, an outside voxel starts   */
/*            from 0.0 and runs steps [fill_after, n_steps).  Not a step kind: */
/*            a rotation takes no program slot.                                */
/*   rounding float64 -> float32 -> fp16, each to nearest even (torch's).     */
/* jobs_host is the table in host memory, jobs_dev the caller's copy of it in */
/* device memory (copied on `stream` before the call); xmap_host / ymap_host  */
/* are the host copies of the device maps.  Nothing is allocated.  Every job  */
/* is validated on the host BEFORE anything is enqueued: a window or a map    */
/* entry outside the source, or an empty extent, is HCU_ERR_SHAPE; more than  */
/* HCU_INGEST_MAX_C channels, more than HCU_AUG_MAX_STEPS steps, or a source  */
/* or destination of 2^31 bytes / elements or more, HCU_ERR_UNSUPPORTED;      */
/* other dtypes, step kinds, channel indices and null pointers                */
/* HCU_ERR_INVALID.  With rot: rot other than 0 / 1, a matrix or offset entry */
/* that is not finite or a matrix entry beyond 1 in magnitude, fill_after      */
/* outside [0, n_steps] is HCU_ERR_INVALID; rot_nx / rot_ny <= 0 or an output  */
/* window (rot_px, ox) / (rot_py, oy) outside the rotated view HCU_ERR_SHAPE.  */
/* Without rot every rot_* field and fill_after must be 0 (HCU_ERR_INVALID).   */
/* ------------------------------------------------------------------------ */
#define HCU_INGEST_MAX_C 16
#define HCU_AUG_MAX_STEPS 8
enum { HCU_AUG_NORMALIZE = 1, HCU_AUG_INTENSITY = 2, HCU_AUG_DROP = 3, HCU_AUG_CLEAN = 4,
       HCU_AUG_GAMMA = 5, HCU_AUG_SPEKLE = 6 };
typedef struct hcu_aug_step {
  int kind;
  unsigned int key;                  /* HCU_AUG_SPEKLE: the noise key */
  double a[HCU_INGEST_MAX_C], b[HCU_INGEST_MAX_C];
} hcu_aug_step;
typedef struct hcu_ingest_job {
  const void *src;                   /* device, [Z][Y][X][C] of src_dtype */
  void *dst;                         /* device, fp16 [n_chan][ox][oy][oz] */
  const int *xmap_dev, *ymap_dev;    /* device int32 [ox] / [oy] ([rot_nx] / [rot_ny] with rot), or null: origin */
  const int *xmap_host, *ymap_host;  /* the same entries in host memory */
  int src_dtype, Z, Y, X, C;
  int ox, oy, oz;                    /* output extent along the source's x, y, z */
  int x0, y0, z0;                    /* window origin (x0 / y0 unused with a map) */
  int n_chan, chan[HCU_INGEST_MAX_C];
  int n_steps;
  double scale;                      /* to_float: 2^-16, 2^-8, or 1 */
  hcu_aug_step steps[HCU_AUG_MAX_STEPS];
  int rot;                           /* 1: rotated gather in the (x, y) plane; 0: every field below is 0 */
  double rot_m[4];                   /* c, s, -s, c (scipy.special.cosdg / sindg of the angle) */
  double rot_off[2];                 /* centre - rot_m @ centre, centre = ((rot_nx - 1) / 2, (rot_ny - 1) / 2) */
  int rot_nx, rot_ny;                /* extents of the pre-rotation view (and of the maps) */
  int rot_px, rot_py;                /* origin of the output window in the rotated view */
  int fill_after;                    /* 0..n_steps: steps that ran before the rotation */
} hcu_ingest_job;
int hcu_ingest_jobs(const hcu_ingest_job *jobs_host, const hcu_ingest_job *jobs_dev, int n_jobs,
                    hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Optimizer. Replaces torch.optim.Adam.step (tests/r_unet_test.py:24,56)   */
/* for a flat parameter buffer: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;  */
/* p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps); L2 weight decay.     */
/* ------------------------------------------------------------------------ */
int hcu_adam_step(float *p, const float *g, float *m, float *v, int64_t n,
                  float lr, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, float grad_scale,
                  hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Per-op entry points (channels-last activations).  Used by the parity     */
/* tests to localise errors; the network executor calls the same kernels.    */
/* ------------------------------------------------------------------------ */
typedef struct hcu_conv_desc {
  int B, Cin, Cout;        /* logical channels                                */
  int X, Y, Z;             /* input spatial dims                              */
  int k[3], stride[3], dil[3];
  int groups;              /* Conv3d only                                     */
  int transposed;          /* 0: nn.Conv3d (valid, stride 1 only)
                              1: nn.ConvTranspose3d (pad 0, dil 1, groups 1) */
  int dtype;               /* HCU_F32: fp32 activations, Cs = round_up(C, 4);
                              HCU_BF16: bf16 activations (x, y, dy, dx),
                              Cs = round_up(C, 8); weights / dw / bias fp32 */
} hcu_conv_desc;

size_t hcu_conv_scratch_bytes(const hcu_conv_desc *d);
/* Output spatial dims of the op described by d (out[3]). */
int hcu_conv_out_dims(const hcu_conv_desc *d, int *out);
/* nn.Conv3d / nn.ConvTranspose3d forward: y = conv(x, w) + bias. */
int hcu_conv_fwd_cl(const hcu_conv_desc *d, const float *x, const float *w,
                    const float *bias, float *y, void *scratch,
                    size_t scratch_bytes, hcu_stream_t stream);
/* d(input) from d(output). */
int hcu_conv_dgrad_cl(const hcu_conv_desc *d, const float *dy, const float *w,
                      float *dx, void *scratch, size_t scratch_bytes,
                      hcu_stream_t stream);
/* d(weight), d(bias) (nullable) from input and d(output); overwrite. */
int hcu_conv_wgrad_cl(const hcu_conv_desc *d, const float *x, const float *dy,
                      float *dw, float *dbias, void *scratch,
                      size_t scratch_bytes, hcu_stream_t stream);

/* nn.MaxPool3d(kernel=stride=k, floor mode) forward, channels-last. */
int hcu_maxpool_fwd_cl(int B, int C, int X, int Y, int Z, const int *k,
                       const float *x, float *y, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Tiled inference (hcat.segment.predict_segmentation_mask, hcat/segment.py:21-136;
 * hcat.utils.pad_image_with_reflections / calculate_indexes, hcat/utils.py:33-124). */
/* ------------------------------------------------------------------------ */
#define HCU_TILE_BATCH_MAX 64
/* out[b][c][i][j][k] = image[0][c][r(o_b + (i,j,k))] for n_tiles tiles of
 * tile_dims, o_b = origins[3b..3b+2] in padded coordinates; r() is numpy's
 * reflection padding (image[pad-1::-1], image, image[-1:-pad-1:-1]) with
 * pad_lo[d] = min(pad, size) (pad_image_with_reflections, utils.py:51-71), and
 * with clean != 0 values are cleaned as segment.py:66-67 does (NaN -> 0,
 * +-Inf -> 1).
 * image: [1][C][X][Y][Z] of image_dtype (HCU_F32 or HCU_F16), device memory;
 * out: [n_tiles][C][tile_dims] fp32, the network input batch. */
int hcu_tile_gather(const void *image, int image_dtype, int C, int X, int Y, int Z,
                    const int *pad_lo, const int *origins, int n_tiles, const int *tile_dims,
                    int clean, float *out, hcu_stream_t stream);
/* mask[dst_lo + w] = f(out[crop_lo + w']) over the write box write_dims, with
 * w' = w or 0 along dimensions where bcast[d] != 0 (torch broadcasting of a
 * size-1 valid_out dimension, segment.py:121-123); out is one channel of one
 * tile's network output [out_dims]; f = the in-place sigmoid chain of
 * segment.py:110-113 (x*-1, exp, +1, pow(-1)), then 1/0 for f > thr when
 * threshold != 0 (segment.py:116-119).  mask: [mask_dims] of HCU_F32 or HCU_U8. */
int hcu_tile_scatter(const float *out, const int *out_dims, const int *crop_lo, const int *bcast,
                     void *mask, int mask_dtype, const int *mask_dims, const int *dst_lo,
                     const int *write_dims, int threshold, float thr, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Training targets from instance labels (hcat/train/train_utils.py: makePWL
 * :9-93, colormask_to_mask :175-187, CalculateCenterOfMass :190-237,
 * VectorToCenter :240-274).  Stacks are [Z][Y][X] (colour stacks
 * [Z][Y][X][3]) with Z*Y*X < 2^31 (HCU_ERR_UNSUPPORTED beyond); results are
 * integers, table values or one float64 division of exact integers, so they
 * are bitwise the reference's.  Every output element is written.            */
/* ------------------------------------------------------------------------ */
#define HCU_PWL_MAX_RADIUS 9
#define HCU_PWL_MAX_OFFSETS (9 * 63)
#define HCU_MOMENT_LDS_IDS 256 /* ids accumulated in LDS by hcu_label_moments */
/* keys[v] = one 64-bit key per voxel: channels 3 (dtype HCU_U8 / HCU_U16),
 * (c0 << 32) | (c1 << 16) | c2, so numeric key order is the lexicographic
 * colour order of np.unique(axis=0); channels 1 (HCU_U8 / HCU_U16 / HCU_I32 /
 * HCU_U32, ids not negative), the id.  map_first != 0: keys equal to voxel
 * 0's become 0 (set_background, :228-237).  Key 0 is background. */
int hcu_label_keys(const void *labels, int dtype, int Z, int Y, int X, int channels, int map_first,
                   uint64_t *keys, hcu_stream_t stream);
/* out[z][y][x] (float64) = makePWL.find_closest (:62-93): 0 where the key is
 * not 0; else the voxel probes, in the same slice, keys[z][y + dy][x + dx]
 * (0 outside the stack: the reference's zero padding) over radii l = 1..9 in
 * order and the offsets of a radius in order; the first key != 0 fixes
 * (closest, l0), the first later key != 0 and != closest fixes l1, and the
 * value is values[(l0 - 1) * 9 + (l1 - 1)], or 0 when either is missing.
 * HOST arrays, copied into the launch: offsets [ring_begin[9]][2] of (dx, dy),
 * each within [-9, 9]; ring_begin [10] ascending from 0 to at most
 * HCU_PWL_MAX_OFFSETS (radius l owns [ring_begin[l-1], ring_begin[l]));
 * values [81] (HCU_ERR_INVALID otherwise). */
int hcu_pwl_scan(const uint64_t *keys, int Z, int Y, int X, const int *offsets, const int *ring_begin,
                 const double *values, double *out, hcu_stream_t stream);
/* moments[id] = {count, sum z, sum y, sum x} over the voxels of each id in
 * [0, n_ids) (voxels with any other value are skipped); moments: [n_ids][4],
 * cleared by the call.  Exact, order-free integer sums. */
int hcu_label_moments(const int32_t *ids, int Z, int Y, int X, int n_ids, uint64_t *moments,
                      hcu_stream_t stream);
/* For each id in [1, n_ids): count[id] = voxels of `center` (HCU_F64, HCU_U8,
 * HCU_U16, HCU_I32 or HCU_U32) equal to id, index[id] = the largest linear
 * index of one, or -1.  index, count: [n_ids], entry 0 is -1 / 0. */
int hcu_center_table(const void *center, int dtype, int Z, int Y, int X, int n_ids, int32_t *index,
                     int32_t *count, hcu_stream_t stream);
/* out[z][y][x][0..2] (float64) = ((z - cz) / Z, (y - cy) / Y, (x - cx) / X)
 * with (cz, cy, cx, use) = centres[4 * id .. 4 * id + 3] (16-byte aligned) of
 * the voxel's id; 0 for id 0, ids outside [0, n_ids) and ids whose `use` is 0. */
int hcu_vector_to_center(const int32_t *ids, int Z, int Y, int X, const int32_t *centres, int n_ids,
                         double *out, hcu_stream_t stream);
/* colormask [Z][Y][X][3] (HCU_U8 / HCU_U16 / HCU_I32 / HCU_U32), in place: a
 * voxel with any channel != 0 becomes (1, 1, 1); mask[z][y][x] (uint8) =
 * channel 0 * 255. */
int hcu_colormask_binary(void *colormask, int dtype, int Z, int Y, int X, uint8_t *mask,
                         hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Instance labels from RDCNet's vector field (hcat/segment.py:
 * pixel_vec_to_cell :563-628, hist3d :631-658).  Volumes are [X][Y][Z], Z
 * contiguous, X*Y*Z < 2^31 (HCU_ERR_UNSUPPORTED beyond).  vec: three channel
 * planes [X][Y][Z] of HCU_F32 / HCU_F16 / HCU_BF16, plane c at vec +
 * c * chan_stride elements (chan_stride >= X*Y*Z: a channel slice of a
 * network output is read in place).  The voxel (x, y, z) points at
 * c = (x + v2, y + v1, z + v0), fp32: the channel order is reversed.
 * Integer atomics only; every float result is bitwise the reference's.     */
/* ------------------------------------------------------------------------ */
#define HCU_VOTE_RADIUS 20 /* taps of hcu_vote_smooth on each side of the centre */
/* counts[floor(c)] += 1 for every voxel whose floor(c) lies inside the volume
 * (compared in fp32; a non-finite component is skipped); max_count[0] =
 * max(max_count[0], largest count).  counts [X*Y*Z] and max_count [1] must be
 * ZERO on entry: the call adds to them.  points != 0: the planes hold the
 * points themselves, c = (plane 0, plane 1, plane 2), and no position is
 * added (hist3d's own argument). */
int hcu_vec_votes(const void *vec, int dtype, int64_t chan_stride, int points, int X, int Y, int Z,
                  uint32_t *counts, uint32_t *max_count, hcu_stream_t stream);
/* hist[v] (float64) = (1 + counts[v]) / (1 + max_count[0]): hist3d's result. */
int hcu_vote_hist(const uint32_t *counts, const uint32_t *max_count, int X, int Y, int Z, double *hist,
                  hcu_stream_t stream);
/* out = gaussian_filter(maximum_filter(hist, size=2, mode='constant'),
 * mode='nearest') of the hist above, float64, over axes 0, 1, 2 in that
 * order.  weights: HOST array [radius + 1], weights[radius] the centre tap,
 * weights[radius - i] the taps at distance i; radius in [0, HCU_VOTE_RADIUS].
 * Each pass sums as scipy's symmetric correlate1d does, t = in[l] * w[r], then
 * for i = r .. 1: t += (in[l-i] + in[l+i]) * w[r-i], indices clamped to the
 * edge, without contraction.  scratch: X*Y*Z float64; out and scratch are
 * both written whole. */
int hcu_vote_smooth(const uint32_t *counts, const uint32_t *max_count, int X, int Y, int Z,
                    const double *weights, int radius, double *out, double *scratch, hcu_stream_t stream);
/* The same three passes over a float64 volume `in` (no maximum filter):
 * stage 3 alone.  in, out and scratch are distinct. */
int hcu_smooth_f64(const double *in, int X, int Y, int Z, const double *weights, int radius, double *out,
                   double *scratch, hcu_stream_t stream);
/* Peak candidates of h (float64, no NaN): voxels off the outermost layer of
 * every axis that equal the maximum of their 3x3x3 neighbourhood and are
 * > min(h).  cand_index[k] (linear index) and cand_value[k] for k <
 * min(*n_found, capacity), in no particular order; *n_found (HOST) = the
 * number found.  state: 4 device words the call owns.  The call WAITS for the
 * stream.  More than `capacity` candidates: HCU_ERR_WORKSPACE, *n_found set. */
int hcu_peak_candidates(const double *h, int X, int Y, int Z, int32_t *cand_index, double *cand_value,
                        int capacity, uint32_t *state, int *n_found, hcu_stream_t stream);
/* label[v] (float64) = label_offset + i of the first peak i (peaks: device
 * int32 [n][3], n >= 0) whose fp32 distance sqrt((c0-p0)^2 + (c1-p1)^2 +
 * (c2-p2)^2) to the voxel's c is strictly below every earlier peak's and
 * below 100000; 0 where none is, and 0 where float(mask[v]) < 0.2 (mask:
 * [X][Y][Z] of HCU_U8, HCU_F32, HCU_F16, HCU_BF16 or HCU_F64; null: no mask). */
int hcu_vec_label(const void *vec, int dtype, int64_t chan_stride, int X, int Y, int Z, const int32_t *peaks,
                  int n, const void *mask, int mask_dtype, int label_offset, double *label,
                  hcu_stream_t stream);
/* One window of a tiled stack (hcunet_amd/instances.py: stitch_vec_to_cell).
 * vec, the peaks and the mask are the window's own, [X][Y][Z], window-local
 * coordinates; dst is the stack's int32 label volume [DX][DY][DZ] (below 2^31
 * voxels too) and (ox, oy, oz) the window's origin in it; the window must lie
 * inside dst (HCU_ERR_SHAPE).  The winner of a voxel is hcu_vec_label's.
 * ids: device int32 [n], the stack-wide id of each peak, 0 for a peak another
 * window owns.  bounds: HOST array {lo0, hi0, lo1, hi1, lo2, hi2} of floats,
 * +-Inf allowed, NaN HCU_ERR_INVALID.  dst[o + v] = ids[winner] iff a peak
 * won, ids[winner] != 0, not float(mask[v]) < 0.2 (null: no mask) and
 * lo_a <= floorf(c_a) < hi_a on every axis (compared as floats); every other
 * voxel of dst is left as it is.  n = 0 writes nothing. */
int hcu_vec_label_paste(const void *vec, int dtype, int64_t chan_stride, int X, int Y, int Z,
                        const int32_t *peaks, const int32_t *ids, int n, const void *mask, int mask_dtype,
                        const float *bounds, int32_t *dst, int DX, int DY, int DZ, int ox, int oy, int oz,
                        hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Cell objects from a label volume (hcat/segment.py: generate_cell_objects
 * :508-560; hcat/haircell.py: HairCell :5-85).  ids: int32 [X][Y][Z], Z
 * contiguous, X*Y*Z < 2^31 (HCU_ERR_UNSUPPORTED beyond), values in
 * [0, n_ids); a voxel with any other value belongs to no id.                */
/* ------------------------------------------------------------------------ */
#define HCU_BOX_LDS_IDS 256      /* ids whose box hcu_cell_boxes keeps in LDS */
#define HCU_CELL_MAX_PLANES 1024 /* largest Z of hcu_cell_stats               */
/* boxes[id] = {x0, y0, z0, x1, y1, z1}: the inclusive minimum and maximum
 * index of the id's voxels along each axis; all six are -1 for an id without
 * a voxel.  boxes: [n_ids][6], every word written.  Integer atomics only. */
int hcu_cell_boxes(const int32_t *ids, int X, int Y, int Z, int n_ids, int32_t *boxes, hcu_stream_t stream);
/* Per id in [1, n_ids) and channel c < C, over the id's CLIPPED box x0:x1,
 * y0:y1, z0:z1 of `boxes` (the maximum face of every axis dropped, as the
 * reference slices; a box is first held inside the volume).  image: C channel
 * volumes [X][Y][Z] of HCU_F32 / HCU_F16 / HCU_BF16, channel c at image +
 * c * chan_stride elements (chan_stride >= X*Y*Z).  Z <= HCU_CELL_MAX_PLANES.
 *   count[id]           voxels of the id in the clipped box
 *   plane_count[id][z]  the same per z plane of the volume (0 outside z0:z1)
 *   box_min[id]         minimum of the clipped box over all C channels and all
 *                       its voxels, the id's or not; NaN when it holds a NaN,
 *                       +inf when it is empty
 *   g                   the channel's values at the id's voxels as float32,
 *                       mapped to g * 0.5f + 0.5f when box_min[id] < 0
 *   mean[id][c]         float64 sum of g / count
 *   std[id][c]          sqrt(sum((g - mean)^2) / count), float64
 *   median[id][c][0..1] the order statistics floor((count - 1) / 2) and
 *                       floor(count / 2) of g (-0 sorts below +0)
 * mean, std and median are NaN where count <= 1 or g holds a NaN.  Row 0 of
 * every table is written as an empty cell's.  The sums are reduced in a fixed
 * order: the same input gives the same bits in every call. */
int hcu_cell_stats(const int32_t *ids, const int32_t *boxes, const void *image, int dtype, int64_t chan_stride,
                   int C, int X, int Y, int Z, int n_ids, int32_t *count, int32_t *plane_count, float *box_min,
                   double *mean, double *std, float *median, hcu_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Measurement: opt-in HIP-event timing of every library launch (bench.py). */
/* ------------------------------------------------------------------------ */
int hcu_timing_enable(int max_launches);
int hcu_timing_disable(void);
/* on != 0: report per network layer ("kernel@layer") instead of per symbol. */
int hcu_timing_detail(int on);
/* Prefix of this thread's launch tags in the detail records (a chain's name,
 * hcunet_amd/chain.py); empty or null: none. */
int hcu_timing_prefix(const char *prefix);
/* One line per kernel symbol: name\tcount\ttotal_ms\tflops\tbytes (totals
 * over launches; flops/bytes are algorithmic).  Returns bytes needed. */
int64_t hcu_timing_report(char *buf, int64_t len);

/* ------------------------------------------------------------------------ */
/* Convolution tiling table.  Plans pick each convolution's tiling from a    */
/* persistent table (tuning/bconv_gfx950.txt next to the library, or         */
/* $HCU_TUNE_FILE) keyed by the convolution's signature, so every process    */
/* and every data-parallel rank runs the same kernels (same summation order). */
/* mode 0: cost model only; 1: table, cost model on a miss (deterministic    */
/* across processes -- hcunet_amd.dist selects it); 2: table, the best few   */
/* candidates timed on a miss (default; $HCU_BCONV_TUNE sets the initial     */
/* mode).                                                                    */
/* ------------------------------------------------------------------------ */
int hcu_tuning_set_mode(int mode);
int hcu_tuning_get_mode(void);
/* Table entries; *timed (nullable) = entries timed by this process. */
int64_t hcu_tuning_entries(int64_t *timed);
/* Writes the table to path (NULL: the library's table file); entries or <0. */
int64_t hcu_tuning_save(const char *path);

#ifdef __cplusplus
}
#endif
#endif /* HCUNET_H */
