/* seg3d_hip.h -- C ABI of libseg3d_hip.so, the MI355X (gfx950) engine behind the segmentation3d plugin API.
 *
 * The reference (qinliuliuqin/Medical-Segmentation3d-Toolkit) has no native boundary: its hot path bottoms out in
 * torch.nn modules.  Each entry point below names the reference call site (file:line under
 * /root/reference/segmentation3d) whose arithmetic it replaces.  The Python host binds these with ctypes
 * (medical-segmentation3d-toolkit_amd/segmentation3d/_engine.py); INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed, e.g. torch.Tensor.data_ptr()) unless noted "host";
 *   - activations are fp32 NDHWC: element (n, z, y, x, c) at (((n*D + z)*H + y)*W + x)*C + c;
 *     probabilities / targets at the plugin API edge are fp32 NCDHW planar ([N][C][S], S = D*H*W);
 *   - weights are passed in the reference layouts (Conv3d [Cout][Cin][k][k][k], ConvTranspose3d [Cin][Cout][k][k][k])
 *     and re-packed on device by seg3d_pack_weights_*;
 *   - `stream` is a hipStream_t (0 = default stream); all work is enqueued on it, nothing synchronises;
 *   - the caller owns every buffer including workspaces (sizes via the *_count / *_floats / *_blocks helpers);
 *     the library keeps no mutable global state, so every call is safe under hipGraph stream capture;
 *   - return value: 0 = ok, <0 = error (SEG3D_ERR_*), message via seg3d_last_error() (thread-local).
 */
#ifndef SEG3D_HIP_H
#define SEG3D_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Adding an entry keeps the version; removing one or changing a prototype raises it.
 * 2: seg3d_adam_step_devstep removed (seg3d_optim_prepare + seg3d_adam_step_ctl do its work). */
#define SEG3D_ABI_VERSION 2

/* ---- library ------------------------------------------------------------------------------------------------ */
const char* seg3d_last_error(void);
int seg3d_abi_version(void);
const char* seg3d_target_arch(void);
int seg3d_device_count(void);

/* ---- layout bridges (utils/image_tools.py:274-326 convert_image_to_tensor / convert_tensor_to_image define the
 *      NCDHW <-> (x,y,z) contract; torch.cat((up, skip), 1) at network/module/vnet_upblock.py:21) ------------------ */
int seg3d_ncdhw_to_ndhwc(const float* in, float* out, int N, int C, long long S, void* stream);
int seg3d_ndhwc_to_ncdhw(const float* in, float* out, int N, int C, long long S, void* stream);
/* dst[v][dst_off + c] = src[v][src_off + c] for c < C, v < nvox; rows of src_ld / dst_ld floats, the other channels of dst
 * are left alone.  Needs src_off + C <= src_ld and dst_off + C <= dst_ld.  Any base, pitch and offset is accepted: the copy
 * moves 16 bytes per access when C, src_ld, src_off, dst_ld and dst_off are all multiples of 4 AND src and dst are both
 * 16-byte aligned, and one float per access otherwise; the result is the same bits either way. */
int seg3d_copy_channels(const float* src, float* dst, long long nvox, int C, int src_ld, int src_off, int dst_ld,
                        int dst_off, void* stream);

/* ---- weight packers: W(a, b, t) = w[a*sa + b*sb + t], a = reduction channel, b = output channel, t = tap ---------- */
int seg3d_pack_weights_tapmajor(const float* w, float* wp, int A, int B, int BP, int T, long long sa, long long sb,
                                int flip, void* stream);
/* MFMA image of one weight tensor (the one-job launch of the multi-pack below; the job is a kernel argument, nothing is
 * allocated).  T = 36 / 48 select the Winograd F(2, 3) / F(2x2, 3x3) images of a 27-tap weight (fp32 only); any other T must
 * be <= 27, the most source taps the packer stages per channel pair: T = 28.. other than 36 / 48 is refused (SEG3D_ERR_INVALID),
 * by seg3d_pack_weights_mfma_bf16 too */
int seg3d_pack_weights_mfma(const float* w, float* wp, int A, int B, int T, long long sa, long long sb, int flip,
                            void* stream);
long long seg3d_packed_mfma_floats(int A, int B, int T);
/* the same pack for many weight tensors in one launch: `jobs_device` is a DEVICE array of njobs descriptors sorted by
 * first_block, first_block[k+1] = first_block[k] + seg3d_pack_job_blocks(A, B, T) of job k; total_blocks = their sum */
typedef struct Seg3dPackJob {
  const float* w;        /* weight tensor (reference layout) */
  float* wp;             /* packed destination, seg3d_packed_mfma_floats(A, B, T) floats */
  long long sa, sb;      /* element strides of the reduction-side / output-side channel in w */
  long long first_block; /* first workgroup of this job */
  int A, B, T, flip;
} Seg3dPackJob;
long long seg3d_pack_job_blocks(int A, int B, int T);
int seg3d_pack_weights_mfma_multi(const Seg3dPackJob* jobs_device, int njobs, long long total_blocks, void* stream);

/* ---- convolutions ---------------------------------------------------------------------------------------------
 * nn.Conv3d k3 s1 p1  : network/module/conv_gn_relu3.py:10, vnet_inblock.py:9, vnet_outblock.py:13
 * nn.Conv3d k2 s2     : network/module/vnet_downblock.py:11
 * nn.Conv3d k1        : network/module/vnet_outblock.py:16
 * nn.ConvTranspose3d k2 s2 : network/module/vnet_upblock.py:11
 * Backward (autograd of the above, core/seg_train.py:124): dgrad = the adjoint op with re-packed weights
 * (k3: same kernel, flipped taps; k2s2 <-> convT), wgrad = seg3d_*_wgrad. */
int seg3d_conv3d_fwd_direct(const float* x, const float* wp_tapmajor, const float* bias, float* y, int N, int Di, int Hi,
                            int Wi, int Cin, int Cout, int ksize, int stride, void* stream);
int seg3d_convT3d_k2s2_fwd_direct(const float* x, const float* wp_tapmajor, const float* bias, float* y, int N, int Di,
                                  int Hi, int Wi, int Cin, int Cout, void* stream);
long long seg3d_wgrad_direct_workspace_floats(int N, int Dq, int Hq, int Wq, int CA, int CB, int ntaps);
int seg3d_wgrad_direct(const float* P, const float* Q, float* part, int N, int Dp, int Hp, int Wp, int CA, int CB,
                       int ksize, int stride, int* n_chunks_out /* host */, void* stream);
int seg3d_wgrad_reduce(const float* part, float* dw, int chunks, int T, int A, int B, long long sa, long long sb,
                       int accumulate /* dw += instead of = */, void* stream);
/* What a weight-gradient call of the VALU fallback family (csrc/conv_direct.hip) runs -- pure host arithmetic: the launchers
 * decide through the same functions.  Arguments as seg3d_wgrad_direct (P's extents) and seg3d_wgrad_reduce.
 *   seg3d_wgrad_direct_variant   0: wgrad_direct_kernel<3, 1, 1>, 1: wgrad_direct_kernel<2, 2, 0>, 2: wgrad_direct_kernel<1, 1, 0>,
 *                                3: wgrad_k1_thin_kernel (ksize 1 with CA <= 8 and CB <= 8).  Negative, with seg3d_last_error set,
 *                                where the launcher refuses: a dimension <= 0, odd extents with stride 2, another (ksize, stride)
 *   seg3d_wgrad_direct_chunks    the partial slabs the launcher writes and reports in n_chunks_out (<= the slabs
 *                                seg3d_wgrad_direct_workspace_floats sizes the workspace for); negative as above
 *   seg3d_wgrad_direct_pairs     PAIRS: the threads of a workgroup that share a voxel, CA * ceil(CB / 4) rounded up to a power of
 *                                two, 256 at most; 256 / PAIRS voxel lanes, gridDim.y = ceil(CA * ceil(CB / 4) / PAIRS)
 *   seg3d_wgrad_reduce_variant   0: wgrad_reduce_kernel, 1: wgrad_reduce_wide_kernel (chunks >= 512 and T * A * B <= 2048) */
int seg3d_wgrad_direct_variant(int N, int Dp, int Hp, int Wp, int CA, int CB, int ksize, int stride);
int seg3d_wgrad_direct_chunks(int N, int Dp, int Hp, int Wp, int CA, int CB, int ksize, int stride);
int seg3d_wgrad_direct_pairs(int CA, int CB);
int seg3d_wgrad_reduce_variant(int chunks, int T, int A, int B);

/* fp32 MFMA implicit-GEMM path for k3 s1 p1 with Cin % 4 == 0 (the FLOP-dominant C->C layers) */
long long seg3d_conv3d_k3_mfma_stats_count(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_mfma_fwd_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
/* kernel instantiation a shape runs: MA (1..4) = conv3d_k3_mfma_kernel<MA>; 100 + 10*MA + NB = conv3d_k3_mfma2_kernel<MA, NB>
 * (conv3d_k3_mfma2_splitk_kernel<MA, NB> + conv3d_splitk_finish_kernel when the workspace query is not 0);
 * 300 + 10*MA + NB = conv3d_k3_mfma2w8_kernel<MA, NB> (8 waves, whole K only) */
int seg3d_conv3d_k3_mfma_variant(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_mfma_fwd(const float* x, const float* wp_mfma, const float* bias,
                             const float* addend /* optional, shape of y: y = conv + bias + addend */, float* y,
                             float* stats_partial, float* workspace /* split-K partials; NULL when the query returns 0 */,
                             int N, int D, int H, int W, int Cin, int Cout, void* stream);
long long seg3d_conv3d_k3_mfma_wgrad_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_mfma_wgrad(const float* x, const float* dy, float* dw, float* workspace, int N, int D, int H, int W,
                               int Cin, int Cout, int accumulate, void* stream);
/* Which kernels of csrc/conv_mfma.hip a weight-gradient call runs (pure host arithmetic: the launchers decide through the
 * same plan functions).  Negative where the launcher would refuse the arguments (a dimension <= 0, Cin % 4 or Cout % 4 != 0,
 * 2^31 elements, fp32: 2^22 tiles).  seg3d_conv3d_k3_mfma_wgrad: bf16 = 0, seg3d_conv3d_k3_bf16_wgrad: bf16 = 1.  10 k + r
 *   k = 0  conv3d_k3_wgrad2_kernel<1, 4, 4, 8>             fp32, the default tile (also every shape no tile divides)
 *   k = 1  conv3d_k3_wgrad2_kernel<1, 4, 4, 4>             fp32, D % 4 == H % 4 == W % 4 == 0 and W % 8 != 0
 *   k = 2  conv3d_k3_wgrad2_kernel<1, 2, 6, 6>             fp32, D % 2 == H % 6 == W % 6 == 0, not whole 4 x 4 x 4 tiles
 *   k = 3  conv3d_k3_wgrad3_bf16_kernel<4, 4, 8, false>    bf16, Cin % 8 == Cout % 8 == 0, whole 4 x 4 x 8 tiles
 *   k = 4  conv3d_k3_wgrad3_bf16_kernel<4, 4, 8, true>     the same tile with ragged extents (IRR)
 *   k = 5  conv3d_k3_wgrad3_bf16_kernel<4, 4, 4, false>    bf16, the 4 x 4 x 4 tile (it covers fewer voxels than 4 x 4 x 8), whole tiles
 *   k = 6  conv3d_k3_wgrad3_bf16_kernel<4, 4, 4, true>     the same tile with ragged extents
 *   k = 7  conv3d_k3_wgrad_mfma_bf16_kernel                bf16, other channel counts: operands widened while staging
 *   r = 1  conv3d_k3_wgrad_reduce_kernel<16> follows (32 or more partial slabs), r = 0  conv3d_k3_wgrad_reduce_kernel<4> */
int seg3d_conv3d_k3_wgrad_variant(int N, int D, int H, int W, int Cin, int Cout, int bf16);

/* bf16 mode (BASELINE config 5: bf16 activations and weights, fp32 accumulation, fp32 GroupNorm statistics, fp32 master
 * weights).  Conv INPUTS (x) and packed weights are bf16 (raw 16-bit patterns, `void*` at this boundary); bias, addend,
 * conv OUTPUT, statistics and workspaces are fp32 as above.  Same nn.Conv3d(k3, p1) call sites (conv_gn_relu3.py:10).
 * Needs Cin % 16 == 0 and Cout % 4 == 0. */
long long seg3d_packed_mfma_bf16_elems(int A, int B, int T);
int seg3d_pack_weights_mfma_bf16(const float* w, void* wp_bf16, int A, int B, int T, long long sa, long long sb, int flip,
                                 void* stream);
/* bf16 images of many weights in one launch; Seg3dPackJob.wp then points at bf16 storage and first_block advances by
 * seg3d_pack_job_blocks_bf16 */
long long seg3d_pack_job_blocks_bf16(int A, int B, int T);
int seg3d_pack_weights_mfma_bf16_multi(const Seg3dPackJob* jobs_device, int njobs, long long total_blocks, void* stream);
int seg3d_f32_to_bf16(const float* src, void* dst_bf16, long long n, void* stream);
int seg3d_bf16_to_f32(const void* src_bf16, float* dst, long long n, void* stream);
/* Winograd F(2, 3) along x form of the same C -> C 3x3x3 convolution (csrc/conv_wino.hip): 2/3 of the fp32 MFMAs, exact
 * fp32 transforms.  wp = seg3d_pack_weights_mfma(A = Cin, B = Cout, T = 36): T = 36 selects the transformed image
 * (t = (kz * 3 + ky) * 4 + p) of the 27-tap weight.  Supported: whole 8 x 8 x 8 tiles, Cin % 8 == 0, Cout % 32 == 0; preferred
 * (the faster choice): also >= 192 (tile, column block) items; other shapes use seg3d_conv3d_k3_mfma_fwd.  replaces nn.Conv3d(C, C, 3, padding=1),
 * network/module/conv_gn_relu3.py:10, and its input gradient (flip = 1, transposed strides) */
int seg3d_conv3d_k3_wino_supported(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino_preferred(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_wino_stats_count(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino_fwd(const float* x, const float* wp_wino, const float* bias, const float* addend, float* y,
                             float* stats_partial, int N, int D, int H, int W, int Cin, int Cout, void* stream);
/* Winograd F(2x2, 3x3) over (y, x) form of the same convolution (csrc/conv_wino2d.hip): a 2 x 2 output quad of one z plane
 * from a 4 x 4 input patch with 16 multiplies instead of 36 per kz = 4/9 of the fp32 MFMAs of the direct kernel; coefficients
 * 1, 1/2, 1/4, exact fp32 transforms.  wp = seg3d_pack_weights_mfma(A = Cin, B = Cout, T = 48): T = 48 selects U = G g G^T per
 * kz (t = kz * 16 + py * 4 + px); the image is opaque to the caller (same size as any T = 48 pack; inside a 32 x 8 chunk it is
 * ordered [4-channel half][group of four K steps][channel][output channel][step] -- the LDS image of the kernels, straight copy).
 * Same arguments as the F(2, 3) form.  Supported: D, H, W multiples of 4 (whole 8^3 tiles run
 * the tile kernel, levels that are only whole 4^3 cells -- the 12^3 level -- the cell kernel), Cin % 8 == 0, Cout % 32 == 0;
 * preferred: at least 192 (tile | group of four cells, 32-channel column block) items.
 * replaces nn.Conv3d(C, C, 3, padding=1), network/module/conv_gn_relu3.py:10, and its input gradient */
int seg3d_conv3d_k3_wino2d_supported(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_preferred(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_wino2d_stats_count(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_fwd(const float* x, const float* wp_wino2d, const float* bias, const float* addend, float* y,
                               float* stats_partial, int N, int D, int H, int W, int Cin, int Cout, void* stream);
/* The same with a caller-owned workspace of seg3d_conv3d_k3_wino2d_fwd_workspace_floats(...) floats (0: none wanted, pass null):
 * launches whose (tile, column block) items would leave more than 6 % of the CU-rounds empty -- 432 items on 256 CUs, the 24^3
 * level of the 4 x 96^3 train step -- deal the K chunks of all items to the workgroups in equal contiguous ranges instead (stream-K);
 * the pieces of an item that a range boundary cuts go through the workspace and a finish pass (one more launch on `stream`).
 * Two calls that run concurrently (two streams) need two workspaces.  Same results up to the order of one fp32 addition per
 * output of a cut item.  replaces nn.Conv3d(C, C, 3, padding=1), network/module/conv_gn_relu3.py:10 */
long long seg3d_conv3d_k3_wino2d_fwd_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_fwd_ws(const float* x, const float* wp_wino2d, const float* bias, const float* addend, float* y,
                                  float* stats_partial, float* workspace, int N, int D, int H, int W, int Cin, int Cout,
                                  void* stream);
/* Winograd F(3, 2) along x form of the weight gradient of the same layers (csrc/conv_wino.hip): 36 point accumulators per
 * (kz, ky, ci block, co block) instead of 27 taps at one voxel PAIR per K slot = 2/3 of the fp32 MFMAs; partial slabs are
 * reduced in fixed order and turned into the three kx taps by the reduce kernel.  Supported: D, H, W multiples of 4, Cin and
 * Cout multiples of 4; dw in the reference layout [Cout][Cin][3][3][3], written or (accumulate != 0) added to.
 * replaces the weight gradient of nn.Conv3d(C, C, 3, padding=1), network/module/conv_gn_relu3.py:10 (autograd) */
int seg3d_conv3d_k3_wino_wgrad_supported(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_wino_wgrad_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino_wgrad(const float* x, const float* dy, float* dw, float* workspace, int N, int D, int H, int W,
                               int Cin, int Cout, int accumulate, void* stream);
/* Winograd F(3x3, 2x2) over (y, x) form of the same weight gradient (csrc/conv_wino2d.hip): 48 accumulators [3 kz][16 points]
 * instead of 27 taps at one output QUAD per K slot = 4/9 of the fp32 MFMAs of the 27-tap kernel; same arguments, shapes and
 * layouts as seg3d_conv3d_k3_wino_wgrad */
int seg3d_conv3d_k3_wino2d_wgrad_supported(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_wgrad_preferred(int N, int D, int H, int W, int Cin, int Cout);   /* else the F(3, 2) form */
long long seg3d_conv3d_k3_wino2d_wgrad_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_wgrad(const float* x, const float* dy, float* dw, float* workspace, int N, int D, int H, int W,
                                 int Cin, int Cout, int accumulate, void* stream);
/* Read-only: which kernels a Winograd launch of this shape runs (tests/wino_cases.py names every one).  Each query calls the
 * function its launcher calls.
 *   seg3d_conv3d_k3_wino2d_fwd_variant     8: conv3d_k3_wino2d_kernel (whole 8^3 tiles), 4 / 2: conv3d_k3_wino2d_c4_kernel with that
 *                                          many 4^3 cells per item (four where that makes 192 items), 0: unsupported
 *   seg3d_conv3d_k3_wino2d_fwd_sk_chunks   K chunks (of four input channels) per workgroup range of the stream-K form that
 *                                          seg3d_conv3d_k3_wino2d_fwd_ws runs when given its workspace; 0: whole items
 *   seg3d_conv3d_k3_wino_wgrad_variant     10 k + r.  k = 0: conv3d_k3_wgrad_wino_kernel<4, 4, 8> (W % 8 == 0), 1: <4, 4, 4>;
 *                                          r = 1: conv3d_k3_wgrad_wino_reduce_kernel<8> (32 slabs or more), 0: <4>
 *   seg3d_conv3d_k3_wino2d_wgrad_variant   10 k + r.  k = 0: conv3d_k3_wgrad_wino2d_kernel;
 *                                          r = 1: conv3d_k3_wgrad_wino2d_reduce16_kernel<16> (64 slabs or more), 0: <4>
 * The weight-gradient queries return -1 for a shape their launcher refuses.  Slabs = workspace floats / (npairs * 36 * 1024)
 * and / (npairs * 48 * 1024), npairs = ceil(Cin / 32) * ceil(Cout / 32) */
int seg3d_conv3d_k3_wino2d_fwd_variant(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_fwd_sk_chunks(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino_wgrad_variant(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_wino2d_wgrad_variant(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_bf16_stats_count(int N, int D, int H, int W, int Cin, int Cout);
long long seg3d_conv3d_k3_bf16_fwd_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
/* 200 + 10*MA + NB = conv3d_k3_mfma2_bf16_kernel<MA, NB> (split-K: conv3d_k3_mfma2_bf16_splitk_kernel<MA, NB> + the finish
 * kernel); 400 + 10*MA + NB = conv3d_k3_mfma2w8_bf16_kernel<MA, NB> (8 waves, whole K only); 0 = shape not supported */
int seg3d_conv3d_k3_bf16_variant(int N, int D, int H, int W, int Cin, int Cout);
/* out_bf16 = 1: y is bf16 storage (used for data-gradients, whose consumer is the GroupNorm backward of a bf16 unit);
 * addend stays fp32 and is added before the rounding */
int seg3d_conv3d_k3_bf16_fwd(const void* x_bf16, const void* wp_bf16, const float* bias, const float* addend, void* y,
                             float* stats_partial, float* workspace, int N, int D, int H, int W, int Cin, int Cout,
                             int out_bf16, void* stream);

/* bf16 mode, remaining conv entry points: the INPUT activations (and, for weight gradients, the output gradient) are
 * bf16 and are widened to fp32 while a tile is staged; weights (fp32 pack), accumulation and outputs are fp32.  Each one
 * mirrors the fp32 entry point of the same name without `bf16` (same call sites in the reference). */
long long seg3d_conv3d_k3_bf16_wgrad_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int seg3d_conv3d_k3_bf16_wgrad(const void* x_bf16, const void* dy_bf16, float* dw, float* workspace, int N, int D, int H,
                               int W, int Cin, int Cout, int accumulate, void* stream);
/* w_bf16 = 1: wp is a seg3d_pack_weights_mfma_bf16(T = 8) image and the kernel runs the bf16 MFMA (Cin % 16 == 0);
 * w_bf16 = 0: fp32 image, the bf16 input is widened while staging */
int seg3d_conv3d_k2s2_bf16_fwd(const void* x_bf16, const void* wp_mfma, const float* bias, void* y, float* stats_partial,
                               int N, int Do, int Ho, int Wo, int Cin, int Cout, int out_bf16, int w_bf16, void* stream);
int seg3d_convT3d_k2s2_bf16_fwd(const void* x_bf16, const void* wp_mfma, const float* bias, void* y,
                                float* stats_partial, int N, int Di, int Hi, int Wi, int Cin, int Cout, int out_bf16,
                                int w_bf16, void* stream);
/* stride-2 conv data-gradient with the skip connection's gradient folded into the epilogue (y = scatter(x) + addend;
 * DownBlock.down_conv = nn.Conv3d(in, out, 2, stride=2), network/module/vnet_downblock.py:11, whose input also feeds
 * torch.cat in vnet_upblock.py:21).  x_mode 0: fp32; 1: bf16 x, fp32 weight image; 2: bf16 x and image */
int seg3d_convT3d_k2s2_scatter_addend(const void* x, int x_mode, const void* wp, const void* addend, int ld_addend, void* y,
                                      int N, int Di, int Hi, int Wi, int Cin, int Cout, int out_bf16, void* stream);
int seg3d_k2_bf16_wgrad(const void* P_bf16, const void* Q_bf16, float* dw, float* workspace, int N, int Dq, int Hq, int Wq,
                        int CA, int CB, long long sa, long long sb, int accumulate, void* stream);
int seg3d_conv3d_k3_thin_out_bf16_fwd(const void* x_bf16, const float* wq, const float* bias, float* y,
                                      float* stats_partial, int N, int D, int H, int W, int Cin, int Cout, int CO,
                                      void* stream);
/* thin-input conv on the bf16 matrix cores (bf16 mode: stem forward CT = 1, head data-gradient CT = 2; Cout % 4 == 0):
 * x fp32 and the weights enter as bf16 hi + lo pairs (three MFMAs per K-step, exact to 2^-16), y is bf16, statistics
 * slots as seg3d_conv3d_k3_thin_in_fwd.  replaces InputBlock.conv = nn.Conv3d(in, 16, 3, padding=1),
 * network/module/vnet_inblock.py:9, and the input gradient of OutputBlock.conv1, vnet_outblock.py:13 */
int seg3d_conv3d_k3_thin_in_mfma16_supported(int CT, int Cout);
long long seg3d_packed_thin_in16_elems(int CT, int B);
int seg3d_pack_weights_thin_in16(const float* w, void* wq_bf16, int CT, int B, long long sa, long long sb, int flip,
                                 void* stream);
int seg3d_conv3d_k3_thin_in_mfma16_fwd(const float* x, const void* wq_bf16, const float* bias, void* y_bf16,
                                       float* stats_partial, int N, int D, int H, int W, int CT, int Cout, void* stream);
/* the same head conv on the matrix cores (Cin in {16, 32}, Cout <= 3): x taps in the reduction dimension, (kz, ky)
 * taps in the output dimension, weights as a bf16 hi + lo pair (fp32-grade); statistics slots as the thin_out kernel.
 * replaces OutputBlock.conv1 = nn.Conv3d(in, out, 3, padding=1), network/module/vnet_outblock.py:13 */
int seg3d_conv3d_k3_thin_out_mfma_supported(int Cin, int Cout);
long long seg3d_thin_out_mfma_packed_elems(int Cin);
int seg3d_pack_weights_thin_out_mfma(const float* w, void* wp_bf16, int A, int B, long long sa, long long sb, int flip,
                                     void* stream);
int seg3d_conv3d_k3_thin_out_mfma_fwd(const void* x_bf16, const void* wp_bf16, const float* bias, float* y,
                                      float* stats_partial, int N, int D, int H, int W, int Cin, int Cout, void* stream);

/* fp32 MFMA path for the stride-2 2x2x2 layers (Cin % 4 == 0): gather = Conv3d k2s2 forward / ConvTranspose3d dgrad,
 * scatter = ConvTranspose3d k2s2 forward / Conv3d k2s2 dgrad, pair-reduce = weight gradient of both.
 * stats_partial: [N][*_stats_count(...)][2] partial (sum, sum of squares) of y; the slots are an opaque order (since round 4:
 * [tile][4 sub-tiles or waves][column block]) -- callers only ever sum a sample's slots (seg3d_gn_stats_finalize) */
long long seg3d_conv3d_k2s2_mfma_stats_count(int Do, int Ho, int Wo, int Cout);
int seg3d_conv3d_k2s2_mfma_fwd(const float* x, const float* wp_mfma, const float* bias, float* y, float* stats_partial,
                               int N, int Do, int Ho, int Wo, int Cin, int Cout, void* stream);
/* x is a channel slice of a wider NDHWC buffer: ld_x floats between consecutive voxel rows (>= Cin, multiple of 4).  Inference:
 * the encoder feature that feeds both the next DownBlock (vnet_downblock.py:11) and a decoder concatenation
 * (vnet_upblock.py:21) is normalised straight into its half of the concatenated buffer and read from there. */
int seg3d_conv3d_k2s2_mfma_fwd_ld(const float* x, int ld_x, const float* wp, const float* bias, float* y, float* stats, int N,
                                  int Do, int Ho, int Wo, int Cin, int Cout, void* stream);
long long seg3d_convT3d_k2s2_mfma_stats_count(int Di, int Hi, int Wi, int Cout);
int seg3d_convT3d_k2s2_mfma_fwd(const float* x, const float* wp_mfma, const float* bias, float* y, float* stats_partial,
                                int N, int Di, int Hi, int Wi, int Cin, int Cout, void* stream);
long long seg3d_k2_mfma_wgrad_workspace_floats(int N, int Dq, int Hq, int Wq, int CA, int CB);
int seg3d_k2_mfma_wgrad(const float* P, const float* Q, float* dw, float* workspace, int N, int Dq, int Hq, int Wq, int CA,
                        int CB, long long sa, long long sb, int accumulate, void* stream);
/* Which kernel instantiation of csrc/conv_k2_mfma.hip a call runs (pure host arithmetic: the launchers decide through the
 * same functions).  Negative where the launcher would refuse the arguments.  x_mode: 0 fp32 x, 1 bf16 x with the fp32 weight
 * image, 2 bf16 x with the bf16 weight image; out_bf16 needs x_mode 1 or 2.
 * gather (seg3d_conv3d_k2s2_mfma_fwd / _fwd_ld / _bf16_fwd): 100 x_mode + 10 out_bf16 + k
 *   k = 0  conv3d_k2s2_mfma_kernel<MODE, OUT_BF>                  LDS-staged: an odd count of 8-channel (mode 2: 16-channel) chunks
 *   k = 1  conv3d_k2s2_direct_kernel<MODE, OUT_BF, NCOB 1, KSPLIT 1>
 *   k = 2  conv3d_k2s2_direct_kernel<MODE, OUT_BF, 2, 1>          Cout % 64 == 0 and at least 16384 waves
 *   k = 3  conv3d_k2s2_direct_kernel<MODE, OUT_BF, 1, 4>          chunk count % 4 == 0 and fewer than 3072 waves
 * scatter (seg3d_convT3d_k2s2_mfma_fwd / _bf16_fwd, and with has_addend seg3d_convT3d_k2s2_scatter_addend):
 *   100 x_mode + 10 out_bf16 + 4 direct + 2 ADD + PAIR
 *   direct = 1  convT3d_k2s2_direct_kernel<MODE, ADD, PAIR>       (fp32 y only)
 *   direct = 0  convT3d_k2s2_mfma_kernel<MODE, OUT_BF, ADD, PAIR>
 *   ADD = has_addend; PAIR = two taps per MFMA (Cout 8 or 16)
 * weight gradient (seg3d_k2_mfma_wgrad: bf16 = 0, seg3d_k2_bf16_wgrad: bf16 = 1): 10 k + r
 *   k = 0  k2_wgrad_mfma_kernel<false>     fp32, CA > 16
 *   k = 1  k2_wgrad_pair_kernel            fp32, CA <= 16
 *   k = 2  k2_wgrad_bf16_mfma_kernel       bf16, CA % 8 == 0 and CB % 8 == 0
 *   k = 3  k2_wgrad_mfma_kernel<true>      bf16, other channel counts
 *   r = 1  k2_wgrad_reduce4_kernel<16> follows (32 or more partial slabs), r = 0  k2_wgrad_reduce_kernel */
int seg3d_conv3d_k2s2_variant(int N, int Do, int Ho, int Wo, int Cin, int Cout, int x_mode, int out_bf16);
int seg3d_convT3d_k2s2_variant(int N, int Di, int Hi, int Wi, int Cin, int Cout, int x_mode, int out_bf16, int has_addend,
                               int ld_addend);
int seg3d_k2_wgrad_variant(int N, int Dq, int Hq, int Wq, int CA, int CB, int bf16);

/* thin 3x3x3 layers at full resolution (stem Cin <= 8 -> 16, head 32 -> num_classes <= 8): HBM-bound special cases
 * of Conv3d k3 p1 (vnet_inblock.py:9, vnet_outblock.py:13) and of their autograd adjoints */
long long seg3d_packed_thin_in_floats(int CT, int B);
int seg3d_pack_weights_thin_in(const float* w, float* wp, int CT, int B, long long sa, long long sb, int flip, void* stream);
long long seg3d_conv3d_k3_thin_stats_count(int D, int H, int W, int Cout_blocks);
int seg3d_conv3d_k3_thin_in_fwd(const float* x, const float* wp_thin, const float* bias, float* y, float* stats_partial,
                                int N, int D, int H, int W, int CT, int Cout, void* stream);
/* bf16 mode: y is bf16 storage (the stem's conv output, the head's data-gradient); everything else as above */
int seg3d_conv3d_k3_thin_in_bf16out_fwd(const float* x, const float* wp_thin, const float* bias, void* y_bf16,
                                        float* stats_partial, int N, int D, int H, int W, int CT, int Cout, void* stream);
int seg3d_pack_weights_thin_out(const float* w, float* wq, int A, int B, int CO, long long sa, long long sb, int flip,
                                void* stream);
long long seg3d_conv3d_k3_thin_out_stats_count(int D, int H, int W);
int seg3d_conv3d_k3_thin_out_fwd(const float* x, const float* wq, const float* bias, float* y, float* stats_partial, int N,
                                 int D, int H, int W, int Cin, int Cout, int CO, void* stream);
/* persistent form of the thin-input conv (csrc/conv_thin_f32.hip): same arithmetic and packed weights as
 * seg3d_conv3d_k3_thin_in_fwd, a workgroup walks tiles with every tile-invariant index hoisted out of the tile loop;
 * statistics: one slot per wave.  y is fp32, or bf16 storage when out_bf16.  replaces InputBlock.conv =
 * nn.Conv3d(in, 16, 3, padding=1), network/module/vnet_inblock.py:9, and the input gradient of OutputBlock.conv1 */
long long seg3d_conv3d_k3_thin_in_persistent_stats_count(int D, int H, int W, int Cout_blocks);
int seg3d_conv3d_k3_thin_in_persistent_fwd(const float* x, const float* wp_thin, const float* bias, void* y,
                                           float* stats_partial, int N, int D, int H, int W, int CT, int Cout, int out_bf16,
                                           void* stream);
/* read-only: the row form the launcher picks from Cout (16 or 32), and grid.x of its tile walk (min(1024 / Cout blocks,
 * tiles)); both call the functions the launcher calls */
int seg3d_conv3d_k3_thin_in_persistent_variant(int Cout);
long long seg3d_conv3d_k3_thin_in_persistent_workgroups(int N, int D, int H, int W, int Cout);
/* fp32 head conv on the fp32 matrix cores (csrc/conv_thin_f32.hip; Cin in {16, 32}, Cout <= 5): x taps in the reduction
 * dimension of v_mfma_f32_16x16x4_f32, (kz, ky) taps in its output rows, the ninth tap on the VALU when 8 taps fill the
 * rows exactly (2 and 4 classes); every voxel row is read once, no LDS staging of activations.  Exact fp32 arithmetic.
 * replaces OutputBlock.conv1 = nn.Conv3d(in, out, 3, padding=1), network/module/vnet_outblock.py:13 */
int seg3d_conv3d_k3_thin_out_f32mfma_supported(int Cin, int Cout);
long long seg3d_thin_out_f32mfma_packed_floats(int Cin, int Cout);
int seg3d_pack_weights_thin_out_f32mfma(const float* w, float* wpk, int A, int B, long long sa, long long sb, int flip,
                                        void* stream);
/* read-only: the z extent of a wave's tile (8, 12, 16, 24, 32 or 48) the launcher's cost model picks */
int seg3d_conv3d_k3_thin_out_f32mfma_tz(int N, int D, int H, int W);
long long seg3d_conv3d_k3_thin_out_f32mfma_stats_count(int N, int D, int H, int W);
int seg3d_conv3d_k3_thin_out_f32mfma_fwd(const float* x, const float* wpk, const float* bias, float* y,
                                         float* stats_partial, int N, int D, int H, int W, int Cin, int Cout, void* stream);
long long seg3d_k3_thin_wgrad_workspace_floats(int N, int D, int H, int W, int CT, int CF);
int seg3d_k3_thin_wgrad(const float* thin, const float* fat, float* dw, float* workspace, int N, int D, int H, int W, int CT,
                        int CF, long long s_ct, long long s_cf, int flip, int accumulate, void* stream);
/* bf16 mode: the same with a bf16 `fat` operand (head weight gradient: fat = the bf16 input activation; stem weight
 * gradient: fat = the bf16 gradient of the conv output).  Runs on the bf16 matrix cores with `thin` split into a bf16
 * hi + lo pair (exact to 2^-17) */
int seg3d_k3_thin_wgrad_fatbf16(const float* thin, const void* fat_bf16, float* dw, float* workspace, int N, int D, int H,
                                int W, int CT, int CF, long long s_ct, long long s_cf, int flip, int accumulate,
                                void* stream);

/* ---- GroupNorm(1, C) [+ ReLU] [+ residual]  (network/module/conv_gn_relu3.py:11,14; residual_block3.py:24,46) ------ */
long long seg3d_gn_stats_count(long long M);
int seg3d_gn_stats_partial(const float* y, float* part, int N, long long M, void* stream);
int seg3d_gn_stats_finalize(const float* part, float* mean_rstd, int N, int count, long long M, float eps, void* stream);
int seg3d_gn_apply(const float* y, const float* mean_rstd, const float* gamma, const float* beta, const float* res,
                   float* out, int N, long long S, int C, int relu,
                   int ld_out /* floats between consecutive voxels of `out`; 0 = C (a channel slice of a wider buffer) */,
                   void* stream);
long long seg3d_gn_bwd_blocks(long long S);
int seg3d_gn_bwd_reduce(const float* dout, const float* out /* NULL: recompute the ReLU mask from y */, const float* y,
                        const float* mean_rstd, const float* gamma, const float* beta, float* part, int N, long long S,
                        int C, int relu, int ld_dout /* row stride of dout in floats, 0 = C */, void* stream);
int seg3d_gn_bwd_finalize(const float* part, const float* gamma, const float* mean_rstd, float* abx, float* s12,
                          float* dgamma, float* dbeta, float* dbias, int N, long long S, int C,
                          int acc_mask /* bit 0/1/2: accumulate into dgamma/dbeta/dbias */, void* stream);
/* both stages in one launch (last-ticket workgroup runs the parameter stage); ticket: one device int, zero before the
 * first call and left zero by every call */
int seg3d_gn_bwd_finalize_fused(const float* part, const float* gamma, const float* mean_rstd, float* abx, float* s12,
                                float* dgamma, float* dbeta, float* dbias, int* ticket, int N, long long S, int C,
                                int acc_mask, void* stream);
int seg3d_gn_bwd_apply(const float* dout, const float* out /* NULL: recompute */, const float* y, const float* mean_rstd,
                       const float* s12, const float* gamma, const float* beta, float* dy, float* dres, int N, long long S,
                       int C, int relu, int ld_dout /* row stride of dout in floats, 0 = C */, void* stream);

/* ReLU mask of a residual unit's output, out = relu(x_in + GN(conv(..))) (residual_block3.py:24,46): the backward pass needs
 * only [out > 0] of the forward output once a residual was added, so the forward apply can write it as one byte per channel
 * quad (bits 0-3 = out > 0 of the quad's four channels; layout [N][S][C/4] bytes, contiguous, 4-byte aligned) and the backward
 * passes read that instead of `out`: g = bit ? dout : 0, everything else (arithmetic, summation order, ld_dout) as in the
 * entries above, results bit-identical.  C % 4 == 0 with C/4 dividing 256 (seg3d_gn_mask_supported). */
int seg3d_gn_mask_supported(int C);
int seg3d_gn_apply_mask(const float* y, const float* mean_rstd, const float* gamma, const float* beta, const float* res,
                        float* out, unsigned char* mask, int N, long long S, int C, int relu, int ld_out, void* stream);
int seg3d_gn_bwd_reduce_mask(const float* dout, const unsigned char* mask, const float* y, const float* mean_rstd,
                             float* part, int N, long long S, int C, int ld_dout, void* stream);
int seg3d_gn_bwd_apply_mask(const float* dout, const unsigned char* mask, const float* y, const float* mean_rstd,
                            const float* s12, const float* gamma, float* dy, float* dres /* optional: the masked dout */,
                            int N, long long S, int C, int ld_dout, void* stream);

/* bf16 mode GroupNorm: the conv output y, the statistics and all arithmetic stay fp32; the activation-side tensors
 * (residual, unit output, incoming gradient) are bf16 where flagged.  ld_out / ld_dout count elements of that tensor. */
/* y_bf16: the conv output y itself is bf16 storage (the conv epilogue rounded it after taking the fp32 statistics) */
int seg3d_gn_apply_mixed(const void* y, const float* mean_rstd, const float* gamma, const float* beta, const void* res,
                         void* out, int N, long long S, int C, int relu, int ld_out, int res_bf16, int out_bf16,
                         int y_bf16, void* stream);
int seg3d_gn_bwd_reduce_bf16(const void* dout_bf16, const void* out_bf16, const void* y, const float* mean_rstd,
                             const float* gamma, const float* beta, float* part, int N, long long S, int C, int relu,
                             int ld_dout, int y_bf16, void* stream);
int seg3d_gn_bwd_apply_bf16(const void* dout_bf16, const void* out_bf16, const void* y, const float* mean_rstd,
                            const float* s12, const float* gamma, const float* beta, void* dy, float* dres, int N,
                            long long S, int C, int relu, int ld_dout, int dy_bf16, int y_bf16, void* stream);

/* ---- head softmax (network/module/vnet_outblock.py:18,23) ---------------------------------------------------------- */
int seg3d_softmax_fwd(const float* in_ndhwc, float* probs_ncdhw, int N, int C, long long S, void* stream);
int seg3d_softmax_bwd(const float* probs_ncdhw, const float* dprobs_ncdhw, float* din_ndhwc, int N, int C, long long S,
                      void* stream);

/* ---- losses: MultiDiceLoss (loss/multi_dice_loss.py:24-43 + loss/binary_dice_loss.py:9-36),
 *              FocalLoss (loss/focal_loss.py:27-61) ------------------------------------------------------------------ */
long long seg3d_dice_blocks(long long S);
int seg3d_dice_fwd(const float* probs, const float* target, const float* weights, float* part, float* sums, float* loss,
                   int N, int C, long long S, void* stream);
int seg3d_dice_bwd(const float* probs, const float* target, const float* sums, const float* weights, const float* gout,
                   float* dprobs, int N, int C, long long S, void* stream);
/* BinaryDiceLoss called on its own (loss/binary_dice_loss.py:9-36): probs [N][2][S], pred = p1 * [p1 > p0] (ties -> 0),
 * float target; part: [N][seg3d_dice_blocks(S)][3], sums: [N][2] (kept for backward), one: device float 1.0f */
int seg3d_binary_dice_fwd(const float* probs, const float* target, const float* one, float* part, float* sums, float* loss,
                          int N, long long S, void* stream);
int seg3d_binary_dice_bwd(const float* probs, const float* target, const float* sums, const float* gout, float* dprobs,
                          int N, long long S, void* stream);
long long seg3d_focal_blocks(long long total_vox);
int seg3d_focal_fwd(const float* probs, const float* target, const float* alpha, float* part, float* loss, int N, int C,
                    long long S, long long sn, long long sc, long long ss, float gamma, int size_average, void* stream);
int seg3d_focal_bwd(const float* probs, const float* target, const float* alpha, const float* gout, float* dprobs, int N,
                    int C, long long S, long long sn, long long sc, long long ss, float gamma, int size_average,
                    void* stream);
/* Compound loss (no counterpart in the reference): L = dice_weight * L_region + ce_weight * L_dist on probabilities
 * [N][C][S] and a float class-id target [N][S].  A voxel counts iff 0 <= t < C and t != ignore_label (pass a value
 * outside [0, C), e.g. -1, for "no ignore label"); every other voxel enters no sum and gets a zero gradient.
 *   L_region = sum_c wdice_c (1 - mean_n d[n,c]),  d = (2 sum p_c t_c + 1e-5) / (sum p_c + sum t_c + 1e-5): soft Dice,
 *              no gate, non-squared denominator; batch_dice != 0 sums over n before the ratio.  wdice: C floats, already
 *              normalised over the included classes, 0 for an excluded class.
 *   L_dist   = sum alpha_t (1 - pt)^gamma (-log pt) / sum alpha_t,  pt = max(p_t, 1e-12); 0 when no voxel counts.
 * A term whose weight is 0 does not enter L.  One pass over probs and target, no atomics, fp64 finalize in fixed order.
 * part: seg3d_compound_loss_part_floats(N, C, S) floats of workspace; loss: 3 floats (L, L_region, L_dist);
 * coef: 2 * R * C + 1 floats kept for the backward, R = batch_dice ? 1 : N -- per (r, c) the pair (A, B) with
 * dL_region/dp[n,c,s] = A t_c + B on counted voxels, then ce_weight / sum alpha_t (0 when that term is off or empty). */
long long seg3d_compound_loss_part_floats(int N, int C, long long S);
int seg3d_compound_loss_fwd(const float* probs, const float* target, const float* wdice, const float* alpha, float* part,
                            float* coef, float* loss, int N, int C, long long S, float gamma, float dice_weight,
                            float ce_weight, int batch_dice, float ignore_label, void* stream);
/* dprobs[n][c][s] = gout[0] * dL/dp: all C planes in one pass, zeros on voxels that do not count; the distribution part
 * sits on the plane c == t and is 0 where p_t < 1e-12 (the clamp's gradient). */
int seg3d_compound_loss_bwd(const float* probs, const float* target, const float* coef, const float* alpha,
                            const float* gout, float* dprobs, int N, int C, long long S, float gamma, int batch_dice,
                            float ignore_label, void* stream);

/* Dice + top-k cross-entropy (no counterpart in the reference; nnU-Net's DC_and_topk_loss):
 * L = dice_weight * L_region + ce_weight * L_topk on probabilities [N][C][S] (fp32, 0 <= p <= 1, 1 <= C <= 16) and a float
 * class-id target [N][S].  A voxel counts iff 0 <= t < C and t != ignore_label (the compound loss's rule, above).
 *   L_region = exactly the compound loss's soft-Dice term (wdice, batch_dice, eps = 1e-5), from the same device code.
 *   ell_v    = alpha_t * (-log(max(p_t, 1e-12))) in fp32 on counted voxels; alpha positive, NOT normalised; -0.0 is +0.0.
 *   n = number of counted voxels of the whole batch; k = max(1, (long long)((double)n * k_percent / 100.0)) for n > 0,
 *       k_percent a double in (0, 100]; n == 0: L_topk = 0, zero gradient, k = 0.
 *   tau = the k-th largest ell (as fp32 values), m = #{ell > tau}, n_eq = #{ell == tau}, r = k - m (1 <= r <= n_eq).
 *   L_topk = (sum_{ell > tau} ell + r * tau) / k.  A term whose weight is 0 does not enter L and sends no gradient.
 *   dL/dp of the top-k term sits on the plane c == t of counted voxels: ce_weight * w_v / k * (p_t >= 1e-12 ? -alpha_t / p_t
 *       : 0), w_v = 1 for ell_v > tau, r / n_eq for ell_v == tau (ties share the remaining r places equally), 0 below.
 * n, k and tau are the calling rank's own: there is no collective.  NaN and p > 1 are outside the contract for values; the
 * kernels stay inside their buffers and terminate on them (their ell is stored as +0.0).
 * tau comes from a three-level radix select (11 / 11 / 10 bits) over the bits of ell, driven by a device control block:
 * integer atomics only (bit-reproducible), nothing is read back, nothing data-dependent is baked into a launch.  The entry
 * zeroes its own counters on the stream at every call, allocates nothing and synchronises nothing, so it can be captured
 * into a hipGraph and replayed on other contents.  N * S must be below 2^32 (the histogram counters).
 * workspace: seg3d_topk_loss_workspace_bytes(N, C, S) bytes, 8-byte aligned, free after the call;
 * ell: N * S floats kept for the backward (a negative sentinel on voxels that do not count);
 * coef: 2 * R * C + 3 floats kept for the backward, R = batch_dice ? 1 : N -- the compound loss's (A, B) pairs, then tau,
 *       ce_weight / k and ce_weight * (r / n_eq) / k (0 when the term is off or nothing counts);
 * loss: 3 floats (L, L_region, L_topk); selection: 5 int64 (n, k, m, n_eq, r); threshold: 1 float, tau. */
long long seg3d_topk_loss_workspace_bytes(int N, int C, long long S);
int seg3d_topk_loss_fwd(const float* probs, const float* target, const float* wdice, const float* alpha, void* workspace,
                        float* ell, float* coef, float* loss, long long* selection, float* threshold, int N, int C,
                        long long S, double k_percent, float dice_weight, float ce_weight, int batch_dice,
                        float ignore_label, void* stream);
/* dprobs[n][c][s] = gout[0] * dL/dp: all C planes in one pass, zeros on voxels that do not count. */
int seg3d_topk_loss_bwd(const float* probs, const float* target, const float* ell, const float* coef, const float* alpha,
                        const float* gout, float* dprobs, int N, int C, long long S, int batch_dice, float ignore_label,
                        void* stream);

/* Dense, batched signed Euclidean distance map of a class-id target (no counterpart in the reference; DESIGN.md section 7,
 * row f16).  target [N][Z][Y][X] float class ids, phi [N][K][Z][Y][X] fp32, class_ids.id[0 .. K-1] the K <= 16 classes.
 * A voxel counts iff 0 <= t < num_class and t != ignore_label (the compound loss's rule; its class is (int)t).  For
 * sample n and class c = class_ids.id[k]:  G = counted voxels of class c,  H = counted voxels of any other class;
 *   phi[n][k](v) = +d(v, G) for v in H,  -d(v, H) for v in G,  0 for a voxel that does not count,
 *   d = sqrt(sx^2 dx^2 + sy^2 dy^2 + sz^2 dz^2) between voxel centres -- the plain signed map edt(~m) - edt(m), WITHOUT the
 *   "- 1" offset of Kervadec's reference code.  G or H empty in a sample: phi[n][k] is 0 everywhere.  Nothing exists outside
 *   the volume, and voxels that do not count are features of no transform (an ignored wall between G and H is no boundary).
 * Exact: three separable passes of out(u) = min_i f(i) + w^2 (u - i)^2 by brute force over the staged line (x, then y, then
 * z), both transforms from one read of each target row; with unit spacing the squared distances are exact integers and
 * |phi| is their correctly rounded fp32 root; otherwise |phi| carries a few fp32 roundings (relative error below 1e-6).
 * Every axis in [1, 256], spacing in [1e-6, 1e6], N * K <= 65535, N * X * Y * Z < 2^31; anything else is an error.
 * workspace: seg3d_signed_distance_workspace_bytes(N, K, X, Y, Z) bytes (two fp32 fields per (n, k)), 4-byte aligned, free
 * after the call.  Allocates nothing, synchronises nothing, reads nothing back: it can be captured into a hipGraph. */
typedef struct Seg3dClassList {
  int id[16];
} Seg3dClassList;
long long seg3d_signed_distance_workspace_bytes(int N, int K, int X, int Y, int Z);
int seg3d_signed_distance(const float* target, float* phi, void* workspace, int N, int X, int Y, int Z,
                          Seg3dClassList class_ids, int K, int num_class, double sx, double sy, double sz,
                          float ignore_label, void* stream);
/* Soft Dice + boundary loss (Kervadec et al., MIDL 2019) on probabilities [N][C][S] (fp32,
 * 1 <= C <= 16, N * S < 2^31), a float class-id target [N][S] and phi [N][C - c0][S] from seg3d_signed_distance for the
 * classes c0 .. C-1 with num_class = C and the same ignore_label (c0 = include_background ? 0 : 1; 16-byte aligned):
 *   L_boundary = sum_c wdice[c] * (sum_{n, counted v} phi[n][c](v) p[n][c](v)) / max(1, n_counted)   (may be negative),
 *   L = dice_weight * L_region + boundary_weight[0] * L_boundary,
 *   L_region = exactly the compound loss's soft-Dice term (wdice, batch_dice, eps = 1e-5), from the same device code and
 *   the same order of additions: bit-equal to seg3d_compound_loss_fwd's loss[1] on the same inputs.
 * wdice: the region weights normalised over the included classes (0 for an excluded background); n_counted: the counted
 * voxels of the whole batch (the calling rank's own: no collective).  boundary_weight is a DEVICE float read by the
 * finalize kernel, so a captured graph follows a schedule that the host writes between replays; dice_weight >= 0.
 * One streaming pass (fp32 partial sums per thread, one slot per workgroup, no atomics) and a one-workgroup fp64 finalize in
 * fixed order: bit-reproducible.  workspace: seg3d_boundary_loss_workspace_bytes(N, C, S) bytes, free after the call;
 * coef: 2 * R * C + C floats kept for the backward, R = batch_dice ? 1 : N -- the compound loss's (A, B) pairs, then per
 * class boundary_weight * wdice[c] / max(1, n_counted);  loss: 3 floats (L, L_region, L_boundary). */
long long seg3d_boundary_loss_workspace_bytes(int N, int C, long long S);
int seg3d_boundary_loss_fwd(const float* probs, const float* target, const float* phi, const float* wdice,
                            const float* boundary_weight, void* workspace, float* coef, float* loss, int N, int C,
                            long long S, float dice_weight, int include_background, int batch_dice, float ignore_label,
                            void* stream);
/* dprobs[n][c][s] = gout[0] * ((A t_c + B) + coef_c * phi[n][c](s)) on counted voxels (no phi part on an excluded background
 * plane), zeros on voxels that do not count: all C planes in one pass.  Neither term's derivative depends on p. */
int seg3d_boundary_loss_bwd(const float* target, const float* phi, const float* coef, const float* gout, float* dprobs, int N,
                            int C, long long S, int include_background, int batch_dice, float ignore_label, void* stream);

/* ---- soft-clDice topology loss (Shit et al., CVPR 2021; no counterpart in the reference) ----
 * Soft skeleton of `planes` fp32 volumes [planes][Z][Y][X] with `iters` = k iterations.  Nothing exists outside the volume:
 *   E(x)(v) = min of x over v and its 6 face neighbours inside the volume,
 *   D(x)(v) = max of x over the 3x3x3 neighbourhood inside the volume,  O(x) = D(E(x)),
 *   x_0 = x, s_0 = relu(x_0 - O(x_0));  for j = 1..k:  x_j = E(x_{j-1}),  d_j = relu(x_j - O(x_j)),
 *   s_j = s_{j-1} + relu(d_j - s_{j-1} d_j);  skel = s_k  -- the published soft_skel.
 * One launch per stage (k + 1 in all): a 32 x 8 x 8 tile with a halo of 2 is staged in LDS, E and D come from there.  Every
 * stage is a selection or one fp32 operation per voxel, so a 0 / 1 volume gives an exact 0 / 1 skeleton.
 * 1 <= iters <= 16, every axis in [1, 256], planes <= 65535, planes * X * Y * Z < 2^31, x != skel; anything else is an error.
 * workspace: seg3d_soft_skeleton_workspace_bytes(planes, X, Y, Z) bytes (two planes' worth of x_j), 4-byte aligned, free
 * after the call.  Allocates nothing, synchronises nothing, reads nothing back: it can be captured into a hipGraph. */
long long seg3d_soft_skeleton_workspace_bytes(long long planes, int X, int Y, int Z);
int seg3d_soft_skeleton(const float* x, float* skel, void* workspace, long long planes, int X, int Y, int Z, int iters,
                        void* stream);
/* Soft Dice + soft-clDice on probabilities [N][C][Z][Y][X] (fp32, 1 <= C <= 16) and a float class-id target [N][Z][Y][X].
 * m(v) = 1 on counted voxels (the compound loss's rule with ignore_label), 0 elsewhere; for sample n and class
 * c = class_ids.id[k], k < K (distinct ids in [0, C)):  P_c = m p_c,  T_c = m [(int)t == c],
 *   SP = skel(P_c), ST = skel(T_c),  Tprec = (sum SP T_c + 1) / (sum SP + 1),  Tsens = (sum ST P_c + 1) / (sum ST + 1),
 *   cl[n][k] = 2 Tprec Tsens / (Tprec + Tsens),  L_cl = sum_k wcl[k] (1 - mean_n cl[n][k])   (batch_dice: the four sums are
 *   summed over n before the ratios),  L = dice_weight * L_dice + cldice_weight * L_cl,
 *   L_dice = exactly the compound loss's soft-Dice term (wdice, batch_dice, eps = 1e-5), from the same device code and the
 *   same order of additions: bit-equal to seg3d_compound_loss_fwd's loss[1] on the same inputs.
 * wdice: the region weights normalised over the included classes (0 for an excluded background); wcl: K weights normalised
 * over the class list.  Term weights >= 0, not both 0; a term whose weight is 0 never enters L (L_cl is still reported).
 * A voxel that does not count is background for both skeletons, enters no sum and gets a zero gradient.
 * Gradient: relu' is 1 for a positive argument, 0 otherwise; a min or max that several positions attain sends its gradient
 * to the one with the lowest linear index (z, then y, then x).  The backward is in gather form -- every voxel collects
 * from the neighbours whose stored selection byte points at it -- in fixed order: no atomics, two runs are bit-equal.
 * Sums: fp32 partials with one slot per workgroup, then a one-workgroup fp64 finalize in fixed order.
 * Limits as for seg3d_soft_skeleton, 1 <= K <= 16, N * K <= 65535, N * X * Y * Z < 2^31.
 * workspace: seg3d_cldice_loss_workspace_bytes(N, C, K, X, Y, Z, iters) bytes, 16-byte aligned; it holds what the backward
 * needs (ST, and per stage and voxel one selection byte and two floats), so the SAME buffer goes to the backward untouched.
 * coef: 2 * R * C + 3 * R * K floats kept for the backward, R = batch_dice ? 1 : N -- the compound loss's (A, B) pairs, then
 * per (r, k) the three factors of the cl term;  loss: 3 floats (L, L_dice, L_cl). */
long long seg3d_cldice_loss_workspace_bytes(int N, int C, int K, int X, int Y, int Z, int iters);
int seg3d_cldice_loss_fwd(const float* probs, const float* target, const float* wdice, const float* wcl, void* workspace,
                          float* coef, float* loss, int N, int C, int X, int Y, int Z, Seg3dClassList class_ids, int K,
                          int iters, float dice_weight, float cldice_weight, int batch_dice, float ignore_label,
                          void* stream);
/* dprobs[n][c][s] = gout[0] * dL/dp[n][c][s] on counted voxels, zeros on voxels that do not count: k + 1 gather passes back
 * through the prediction's skeleton (none when cldice_weight is 0), then all C planes in one pass.  Same arguments as the
 * forward call whose workspace and coef it gets. */
int seg3d_cldice_loss_bwd(const float* target, void* workspace, const float* coef, const float* gout, float* dprobs, int N,
                          int C, int X, int Y, int Z, Seg3dClassList class_ids, int K, int iters, float cldice_weight,
                          int batch_dice, float ignore_label, void* stream);

/* ---- region-based models (no counterpart in the reference) -----------------------------
 * Head sigmoid: the counterparts of the soft-max pair above, same layouts (NDHWC in, contiguous NCDHW out), 1 <= C <= 16.
 * p = 1 / (1 + exp(-x)) evaluated through exp(-|x|): finite and inside [0, 1] for every x.  Backward: din = dp p (1 - p). */
int seg3d_sigmoid_fwd(const float* in_ndhwc, float* probs_ncdhw, int N, int C, long long S, void* stream);
int seg3d_sigmoid_bwd(const float* probs_ncdhw, const float* dprobs_ncdhw, float* din_ndhwc, int N, int C, long long S,
                      void* stream);

/* Region loss (no counterpart in the reference): soft Dice + binary cross-entropy / focal on
 * the sigmoid probabilities of a region-based model.  The stock-torch chain it stands for is a table gather of R binary
 * targets, 3 R masked sums and F.binary_cross_entropy.  probs [N][R][S] planar fp32 (1 <= R <= 16), target [N][S] float label
 * ids, lut_host: 256 HOST words, bit r of lut_host[l] set iff label l is in region r (copied into the kernel arguments, so
 * a captured graph keeps the table it was captured with).
 *   counting rule: l = the integer in [0, 256) that t is, else -1; a voxel counts iff l >= 0 && t != ignore_label (any
 *             ignore_label outside [0, 256) means none).  A voxel that does not count enters no sum and gets gradient 0 on
 *             every plane.  The target of region r is z_r = (lut[l] >> r) & 1: a label in no region is background everywhere.
 *   L_dice  = the compound loss's soft-Dice term with planes as classes, from the same device code: I = sum p z, P = sum p,
 *             T = sum z over counted voxels, d[n,r] = (2 I + 1e-5) / (P + T + 1e-5), sum_r wdice_r (1 - mean_n d[n,r]);
 *             wdice: R floats normalised over the regions; batch_dice != 0 sums over n before the ratio.
 *   L_bce   = sum_v sum_r alpha_r l_r / (n_counted sum_r alpha_r), 0 when nothing counts;  q = z ? p : 1 - p,
 *             l_r = (1 - qc)^gamma (-log qc), qc = max(q, 1e-12): one logarithm per plane and voxel.  With unit alpha and
 *             gamma = 0 this is F.binary_cross_entropy(p, z) (mean) over the counted voxels.
 *   L = dice_weight * L_dice + bce_weight * L_bce, both weights >= 0 and not both 0; a term whose weight is 0 does not
 *   enter L.  One pass over probs and target, no atomics, fp64 finalize in fixed order: bit-reproducible, capturable.
 * part: seg3d_region_loss_part_floats(N, R, S) floats of workspace ([N][blocks][3 R + 2]: the (I, P, T) triples, the BCE
 * numerator, the counted voxels); loss: 3 floats (L, L_dice, L_bce); coef: 2 * Rd * R + 1 floats kept for the backward,
 * Rd = batch_dice ? 1 : N -- the pairs (A, B) of seg3d_compound_loss_fwd, then bce_weight / (n_counted sum_r alpha_r). */
long long seg3d_region_loss_part_floats(int N, int R, long long S);
int seg3d_region_loss_fwd(const float* probs, const float* target, const unsigned* lut_host, const float* wdice,
                          const float* alpha, float* part, float* coef, float* loss, int N, int R, long long S, float gamma,
                          float dice_weight, float bce_weight, int batch_dice, float ignore_label, void* stream);
/* dprobs[n][r][s] = gout[0] * [(z ? A + B : B) + coef_bce alpha_r d/dq[(1 - q)^gamma (-log q)] (z ? 1 : -1)] on counted
 * voxels, 0 elsewhere; the BCE part is 0 where q < 1e-12 (the clamp's gradient).  All R planes in one pass. */
int seg3d_region_loss_bwd(const float* probs, const float* target, const unsigned* lut_host, const float* coef,
                          const float* alpha, const float* gout, float* dprobs, int N, int R, long long S, float gamma,
                          int batch_dice, float ignore_label, void* stream);

/* ---- deep supervision (no counterpart in the reference): auxiliary heads on the lower decoder levels + label pyramid -- */
/* Fused head: what nn.Conv3d(Cin, C, 1) + nn.Softmax(dim=1) compute on a decoder feature, in one streaming pass.
 *   x: NDHWC fp32 rows [N * S][Cin] at a row stride of ldx floats (0 = Cin; else a multiple of 4 >= Cin: a channel slice of
 *      a wider buffer is read in place), 16-byte aligned;  w: [C][Cin] (the Conv3d weight seen flat, no packing);  b: [C] or
 *      NULL;  probs: contiguous NCDHW [N][C][S], p = softmax_c(w x + b) with the max subtracted as in seg3d_softmax_fwd.
 * Supported (seg3d_ds_head_supported): Cin % 4 == 0, Cin <= 256, 1 <= C <= 8; anything else returns an error. */
int seg3d_ds_head_supported(int Cin, int C);
int seg3d_ds_head_fwd(const float* x, int ldx, const float* w, const float* b, float* probs, int N, long long S, int Cin,
                      int C, void* stream);
/* Backward of the fused head: g_c = p_c (dp_c - sum_k p_k dp_k);  dx[v][ci] = sum_c g_c w[c][ci] written as NDHWC rows at
 * a row stride of ld_dx floats (0 = Cin);  per-workgroup partial sums of dw[c][ci] = sum_v g_c x[v][ci] and
 * db[c] = sum_v g_c go to `workspace` (seg3d_ds_head_bwd_workspace_floats floats; a pure function of the shape).  x is
 * read once, dx written once, no atomics. */
long long seg3d_ds_head_bwd_workspace_floats(int N, long long S, int Cin, int C);
int seg3d_ds_head_bwd(const float* probs, const float* dprobs, const float* x, int ldx, const float* w, float* dx, int ld_dx,
                      float* workspace, int N, long long S, int Cin, int C, void* stream);
/* Adds the partials of seg3d_ds_head_bwd (same N, S, Cin, C, same device) in a fixed order in fp64 and writes dw [C][Cin]
 * and db [C] (either may be NULL); accumulate: bit 0 -- ADD into dw instead of overwriting it, bit 1 -- the same for db
 * (the optimizer's gradient sinks).  Bit-reproducible. */
int seg3d_ds_head_bwd_finalize(const float* workspace, float* dw, float* db, int N, long long S, int Cin, int C,
                               int accumulate, void* stream);
/* Label pyramid: one launch writes out_k[n][z][y][x] = mask[n][f z][f y][f x], f = 2^k, for k = 1..levels (levels <= 3;
 * out_k contiguous [N][D/f][H/f][W/f], outputs past `levels` may be NULL).  Values are copied, not interpreted.  D, H, W
 * must be divisible by 2^levels. */
int seg3d_label_pyramid(const float* mask, float* out1, float* out2, float* out3, int N, int D, int H, int W, int levels,
                        void* stream);

/* ---- optimizer: optim.Adam(...).step()  (core/seg_train.py:83,127) --------------------------------------------------
 * One call with every scalar a launch argument; step >= 1 counts the step being taken.  A train step captured in a
 * hipGraph cannot change a launch argument: keep the count on the device with seg3d_optim_prepare (CONSTANT schedule,
 * max_norm 0) + seg3d_adam_step_ctl below, which give the same bits. */
int seg3d_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step, float lr,
                    float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* ---- optimizer control block: gradient-norm clipping, learning-rate schedules, SGD (no counterpart in the reference) ---
 * The per-step scalars live on the device so that a step captured in a hipGraph can change them and the gradient norm
 * never travels to the host.  One step of a parameter group is
 *     [seg3d_grad_sumsq_partial, only when clipping]  ->  seg3d_optim_prepare  ->  seg3d_sgd_step_ctl | seg3d_adam_step_ctl
 * Control block: SEG3D_CTL_FLOATS floats, written by seg3d_optim_prepare, read by the *_ctl updates:
 *   [SEG3D_CTL_LR]         learning rate of this step
 *   [SEG3D_CTL_GRAD_MULT]  gradient multiplier grad_scale * coef (exactly grad_scale when coef == 1)
 *   [SEG3D_CTL_BC1]        Adam: 1 - beta1^t
 *   [SEG3D_CTL_BC2_SQRT]   Adam: sqrt(1 - beta2^t)
 *   [SEG3D_CTL_NORM]       grad_scale * sqrt(sum of squares): the global gradient norm (0 when max_norm <= 0)
 *   [SEG3D_CTL_COEF]       clip coefficient min(1, max_norm / (norm + 1e-6))  (1 when max_norm <= 0)
 *   [6], [7]               reserved */
#define SEG3D_CTL_LR 0
#define SEG3D_CTL_GRAD_MULT 1
#define SEG3D_CTL_BC1 2
#define SEG3D_CTL_BC2_SQRT 3
#define SEG3D_CTL_NORM 4
#define SEG3D_CTL_COEF 5
#define SEG3D_CTL_FLOATS 8
#define SEG3D_SCHEDULE_CONSTANT 0
#define SEG3D_SCHEDULE_POLY 1
#define SEG3D_SCHEDULE_COSINE 2
/* sum of squares of n floats (16-byte aligned): part[b] = fp64 partial of workgroup b, b < seg3d_grad_sumsq_part_count(n)
 * (host arithmetic, at most 8192).  Exact fp64 products, fp64 accumulation, no atomics; the summation order depends on n
 * only, so two calls on the same data are bit-equal. */
long long seg3d_grad_sumsq_part_count(long long n);
int seg3d_grad_sumsq_partial(const float* grads, long long n, double* part, void* stream);
/* one workgroup: t = *step_dev + 1 (stored back); with max_norm > 0 the nparts slots (of all parameter groups, laid end
 * to end) are added in a fixed order in fp64 and norm / coef follow the rule above -- torch.nn.utils.clip_grad_norm_'s,
 * including that a non-finite norm is not skipped; with max_norm <= 0 the slots are not read (part may be NULL).
 * Learning rate, with s = t - 1 completed steps, T = total_steps, in fp64 and rounded once to float:
 *   lr = base_lr * w(s) * d(s),  w = warmup_steps ? min(1, (s + 1) / warmup_steps) : 1,
 *   d = 1 (CONSTANT) | max(0, 1 - s / T)^power (POLY) | 0.5 (1 + cos(pi min(s, T) / T)) (COSINE)
 * beta1 / beta2 feed Adam's bias corrections only (pass 0 for SGD). */
int seg3d_optim_prepare(int* step_dev, float* ctl, const double* part, int nparts, float grad_scale, float max_norm,
                        int schedule, float base_lr, int total_steps, int warmup_steps, float power, float beta1,
                        float beta2, void* stream);
/* torch.optim.SGD with dampening 0:  g = grads * ctl.mult + weight_decay * p;  buf = momentum * buf + g;
 * d = nesterov ? g + momentum * buf : buf;  p -= ctl.lr * d.  A zero-initialised buf makes the first step torch's buf = g.
 * momentum == 0: momentum_buf is neither read nor written (may be NULL). */
int seg3d_sgd_step_ctl(float* params, const float* grads, float* momentum_buf, long long n, const float* ctl,
                       float momentum, float weight_decay, int nesterov, void* stream);
/* seg3d_adam_step with lr, the gradient multiplier and the bias corrections read from the control block */
int seg3d_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                        const float* ctl, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- sliding-window batcher (core/seg_infer.py:208-246, 313-327, 336-339; utils/image_tools.py:435-469;
 *      utils/normalizer.py:6-81) ---------------------------------------------------------------------------------- */
long long seg3d_patch_stats_blocks(int bx, int by, int bz);
/* the M = 1 case of seg3d_patch_gather_normalize_mc below: volume [Z][Y][X] -> batch [P][1][bz][by][bx], the same memory as
 * [Z][Y][X][1] -> [P][bz][by][bx][1].  normalizer_type 0 = fixed (mean, stddev, clip to [-1, 1] when clip != 0),
 * 1 = adaptive (clip to +-clip_sigma, clip_sigma > 0), -1 = none.  workspace: P * seg3d_patch_stats_blocks * 2 doubles,
 * mean_std: P * 2 floats (adaptive only) -- the M = 1 sizes of the _mc entry. */
int seg3d_patch_gather_normalize(const float* volume, const int* starts_xyz, float* batch, double* workspace,
                                 float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P, int normalizer_type,
                                 float mean, float stddev, int clip, float clip_sigma, void* stream);
/* M co-registered modalities (1 <= M <= 8), channels-last volume [Z][Y][X][M] -> batch [P][bz][by][bx][M] (NDHWC of
 * the patch batch).  Replaces the per-modality crop + crop_normalizers[idx] of dataset.py:199-203 and the
 * crop_normalizers[0]-only ROI normalisation of core/seg_infer.py:221-224.  One normaliser per modality, passed by
 * value: type 0 = fixed ((x - mean) / stddev, clipped to [clip_lo, clip_hi] when clip != 0), 1 = adaptive (the patch's
 * own fp64 mean / population std floored at 1e-6, clipped to [clip_lo, clip_hi]), -1 = none.  Channel m is
 * bit-identical to the M = 1 gather of plane m with normaliser m.  starts / control-block contract of the scatter below;
 * no host sync, no allocation (capturable).  workspace: seg3d_patch_stats_mc_doubles doubles; mean_std: P * M * 2
 * floats (adaptive only). */
typedef struct Seg3dNormalizer {
  int type;
  float mean, stddev;
  int clip;
  float clip_lo, clip_hi;
} Seg3dNormalizer;
typedef struct Seg3dNormalizers {
  Seg3dNormalizer n[8];
} Seg3dNormalizers;
long long seg3d_patch_stats_mc_doubles(int bx, int by, int bz, int P, int M);
int seg3d_patch_gather_normalize_mc(const float* volume, const int* starts_xyz, float* batch, double* workspace,
                                    float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P, int M,
                                    Seg3dNormalizers norms, void* stream);
/* the wtab = NULL, flip_mask = 0 case of seg3d_patch_scatter_blend below: probs [P][C][bz][by][bx] of the ctl[6] valid
 * patches are added to acc [C][Z][Y][X] in list order and count [Z][Y][X] grows by 1.0f per covering patch */
int seg3d_patch_scatter_accumulate(const float* probs, const int* starts_xyz, const int* ctl /* device int32[7] */,
                                   float* acc, float* count, int Z, int Y, int X, int bx, int by, int bz, int C,
                                   long long max_box_voxels, void* stream);
int seg3d_finalize_argmax(float* acc, const float* count, signed char* mask, int C, long long voxels,
                          long long class_stride, void* stream);
/* Region-based inference: acc[r][v] *= 1 / count[v] in place (R region planes, class_stride and z-slab convention as
 * above), then mask = 0 and for r = 0 .. R-1 in order: p_r > 0.5 (strictly) sets mask = order_host[r] -- the sequential
 * overwrite rule, so regions are listed from the largest to the smallest.  order_host: R host ints in 1..127.  A voxel
 * with count 0 gets probabilities 0 and mask 0.  mask may be NULL. */
int seg3d_finalize_regions(float* acc, const float* count, signed char* mask, int R, const int* order_host,
                           long long voxels, long long class_stride, void* stream);
/* ---- Gaussian patch blending and mirror test-time augmentation ---------------------------
 * flip_mask: bit 0 = x, bit 1 = y, bit 2 = z, 0..7.
 * The _flip gathers are the gathers above with every patch mirrored: batch element (lz, ly, lx) of patch p is the
 * normalised volume voxel at start_p + (fx ? bx-1-lx : lx, fy ? by-1-ly : ly, fz ? bz-1-lz : lz).  The adaptive
 * normaliser's mean / std are those of the un-mirrored patch bit for bit, so the result equals the flipped plain gather
 * exactly.  A mirrored gather cannot run in place.  seg3d_patch_gather_normalize_flip is the M = 1 case of
 * seg3d_patch_gather_normalize_mc_flip, and flip_mask = 0 is the plain gather.
 * seg3d_patch_scatter_blend: the accumulation with a weight per local voxel and mirrored inputs.
 * wtab: device, bx + by + bz floats = the x, y and z tables one after the other (NULL = weight 1); the weight of local
 * voxel (lx, ly, lz) is the float32 w = (g_z[lz] * g_y[ly]) * g_x[lx]; acc[c][v] = acc[c][v] + (w * prob) and
 * count[v] = count[v] + w with a rounded multiply and a rounded add (no FMA), patches in list order, no atomics.  The
 * probabilities of patch p are stored mirrored by flip_mask (the output of a net that was fed the _flip gather) and are
 * accumulated un-mirrored.  wtab = NULL and flip_mask = 0 is seg3d_patch_scatter_accumulate (w = 1: the product is the
 * probability itself).
 * All three: no allocation, no host sync, control block on the device (capturable). */
int seg3d_patch_gather_normalize_flip(const float* volume, const int* starts_xyz, float* batch, double* workspace,
                                      float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P,
                                      int normalizer_type, float mean, float stddev, int clip, float clip_sigma,
                                      int flip_mask, void* stream);
int seg3d_patch_gather_normalize_mc_flip(const float* volume, const int* starts_xyz, float* batch, double* workspace,
                                         float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P, int M,
                                         Seg3dNormalizers norms, int flip_mask, void* stream);
int seg3d_patch_scatter_blend(const float* probs, const int* starts_xyz, const int* ctl /* device int32[7] */,
                              const float* wtab, float* acc, float* count, int Z, int Y, int X, int bx, int by, int bz,
                              int C, int flip_mask, long long max_box_voxels, void* stream);

/* ---- model ensembling on the image grid (not in the reference) ---------------------------
 * One launch per ensemble member: its finalized probabilities src [C][Zi][Yi][Xi] (planar, on the member's own grid) are
 * interpolated onto the image grid and added with the member's weight into acc [C][Zo][Yo][Xo].  For an output voxel v
 * and plane c:
 *   s_c = what seg3d_resample_affine(src_c, .., affine_host, linear = 1, pad) writes at v, bit for bit, with pad = pad0
 *         for c = 0 and 0 otherwise (the coordinate, the inside test and the weights are computed once per voxel and
 *         shared by the C planes);
 *   a_c = first ? weight * s_c : acc_c + weight * s_c in fp32, a rounded multiply and a rounded add (no FMA);
 *         acc_c = a_c.  With `first` acc is not read, so the caller need not clear it.
 * mask (int8 [Zo][Yo][Xo]; NULL on every member but the last) is written from the a_c of the same pass:
 *   order_host == NULL: mask = argmax_c a_c, first maximum wins (the rule of seg3d_finalize_argmax);
 *   order_host != NULL (C host ints in 1..127): mask = 0, then for r = 0 .. C-1 in order a_r > 0.5 (strictly) writes
 *   order_host[r] (the rule of seg3d_finalize_regions).
 * The caller normalises the weights to sum 1, so acc after the last member is the mean: there is no scale pass.
 * 1 <= C <= 16.  affine_host: 12 doubles on the HOST, as seg3d_resample_affine.  16-byte accesses when Xo % 4 == 0 and acc
 * is 16-byte (mask 4-byte) aligned, a scalar path otherwise; no workspace, no host sync. */
int seg3d_ensemble_accumulate(const float* src, float* acc, signed char* mask, int C, int Xi, int Yi, int Zi, int Xo,
                              int Yo, int Zo, const double* affine_host, float weight, int first, float pad0,
                              const int* order_host, void* stream);

/* ---- evaluation metric: utils/metrics.py:5-37 cal_dsc, core/seg_eval.py:8-57 ---------------
 * counts[3k..3k+2] += (area_gt, area_seg, intersection) of labels_host[k] over two label volumes of n elements;
 * the caller zeroes counts first.  dtype: 0 int8, 1 uint8, 2 int16, 3 int32, 4 float32.  1..16 labels per call. */
int seg3d_label_overlap_counts(const void* gt, const void* seg, int dtype, long long n, const int* labels_host, int nlabels,
                               unsigned long long* counts, void* stream);

/* The same with set membership: counts[3r..3r+2] += (|gt in region r|, |seg in region r|, |both|).  lut_host: 256 host
 * words, bit r of lut_host[l] set iff label l is in region r; a value that is no integer in [0, 256) is in no region.
 * 1..16 regions per call, the same five dtypes, integer counting. */
int seg3d_region_overlap_counts(const void* gt, const void* seg, int dtype, long long n, const unsigned* lut_host,
                                int nregions, unsigned long long* counts, void* stream);

/* ---- online validation: arg-max + per-class confusion counts in one pass ---------------
 * Replaces nothing in the reference (its core/seg_train.py has no validation); the stock-torch chain it stands for is
 * probs.argmax(1) followed by 3 C masked sums.  probs [N][C][S] planar fp32, target [N][S] float class ids, 1 <= C <= 16.
 * A voxel counts iff t >= 0 && t < C && t != ignore_label (the rule of seg3d_compound_loss_fwd; any value outside [0, C)
 * means "no ignore label"); its prediction is the FIRST maximum over the classes (class 0, replaced only by a strictly
 * greater value).  counts[3c..3c+2] += (tp, fp, fn) of class c: the caller owns and zeroes the 3 * C device int64 words, so
 * a whole validation pass accumulates on the device.  Integer arithmetic only (bit-exact in any order); no allocation and
 * no synchronisation, so the call can be captured into a hipGraph. */
int seg3d_confusion_counts(const float* probs, const float* target, long long* counts, int N, int C, long long S,
                           float ignore_label, void* stream);
/* The same for a region-based model (row f23; stands for R thresholds and 3 R masked sums in stock torch): probs [N][R][S]
 * sigmoid probabilities, the prediction of region r is p_r > 0.5 STRICTLY (the rule of seg3d_finalize_regions), its target
 * bit r of lut[l], and a voxel counts by the rule of seg3d_region_loss_fwd.  counts[3r..3r+2] += (tp, fp, fn) of region r
 * into 3 * R caller-owned device int64 words.  lut_host: 256 host words.  Integer arithmetic only, at most 3 R 64-bit
 * integer atomics per workgroup; no allocation and no synchronisation. */
int seg3d_region_confusion_counts(const float* probs, const float* target, const unsigned* lut_host, long long* counts, int N,
                                  int R, long long S, float ignore_label, void* stream);

/* ---- surface-distance metrics: HD, HD95, ASSD of one label --------------------------------
 * seg3d_label_surface: surface[i] = 1 on the voxels of (labels == label) that have a 6-neighbour outside the label
 * (voxels outside the volume count as outside), else 0, over an X x Y x Z volume ([Z][Y][X], < 2^31 voxels, dtype as
 * above).  box_device[6] = inclusive (xmin, ymin, zmin, xmax, ymax, zmax), initialised by the caller to
 * {INT_MAX x3, -1 x3}, is widened to the surface voxels; count_device[0] += their number.  Call it for the ground truth
 * and the segmentation with ONE box: it then encloses both surfaces.
 * seg3d_surface_distance: for every voxel of query_surface inside the box, the squared Euclidean distance (physical
 * units, spacing (sx, sy, sz)) from its centre to the nearest centre of a feature_surface voxel, by an exact separable
 * EDT over the box only.  The squared distances go compacted, in no fixed order, to dist2_out[0 .. capacity) with the
 * linear voxel index in index_out (may be NULL); stats[3] = (count, max distance, sum of distances), the sum in fp64 and
 * reduced in a fixed order.  Squared distances are exact for unit spacing.  workspace:
 * seg3d_surface_distance_workspace_bytes (-1: bad size); no host sync, no allocation (capturable). */
int seg3d_label_surface(const void* labels, int dtype, int X, int Y, int Z, int label, unsigned char* surface,
                        int* box_device, int* count_device, void* stream);
long long seg3d_surface_distance_workspace_bytes(int X, int Y, int Z);
int seg3d_surface_distance(const unsigned char* feature_surface, const unsigned char* query_surface, int X, int Y, int Z,
                           const int* box_device, double sx, double sy, double sz, void* workspace, double* dist2_out,
                           int* index_out, long long capacity, double* stats, void* stream);

/* ---- pre/post-processing around the patch path: utils/image_tools.py:329-432, 481-510 ----------
 * resample: dst[z][y][x] (Xo, Yo, Zo) = src sampled at the continuous index c = M * (x, y, z, 1), M = 12 doubles on the
 * HOST (row-major 3 x 4); ITK semantics: inside iff -0.5 <= c < size - 0.5, else `pad`; linear (clamped 8-neighbourhood)
 * or nearest neighbour (round half up).  seg3d_resample_affine is the M = 1, dst_stride = 1 case of
 * seg3d_resample_affine_mc. */
int seg3d_resample_affine(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                          const double* affine_host, int linear, float pad, void* stream);
/* the same resampling for M co-registered channels sharing one geometry (dataset.py:199-203 crops every modality at
 * one centre and spacing; core/seg_infer.py:221-224 + image_tools.py:348-377 resample the case to the model spacing):
 * src [Zi][Yi][Xi][M], output voxel (x, y, z) written as M floats at dst + ((z * Yo + y) * Xo + x) * dst_stride
 * (dst_stride >= M; a crop goes straight into slot b of an NDHWC batch).  Channel m is bit-identical to the M = 1
 * resampling of plane m.  1 <= M <= 8. */
int seg3d_resample_affine_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi, int Xo,
                             int Yo, int Zo, const double* affine_host, int linear, float pad, void* stream);
/* ---- training augmentation (not in the reference) -----------------------------------------
 * The two resampling entries with an elastic deformation of the sampled point:
 *   c = M (x, y, z, 1) + L u(x', y', z'),  L = l_host, 9 doubles on the HOST (row-major 3 x 3, diag(1 / s_src) D_src^-1),
 * u a displacement in millimetres (world axes): the tensor-product cubic B-spline over the control grid
 * ctrl [gz][gy][gx][3] (DEVICE, float32, components x, y, z) laid over the destination grid.  Per axis a of n voxels with
 * t_host[a] = crop spacing / control spacing (3 doubles on the HOST, each in [0, 1]): t = i * t_host[a], k = floor(t),
 * f = t - k, u = sum_{j = 0..3} B_j(f) ctrl[k + j] with the uniform cubic basis B_0 = (1 - f)^3 / 6,
 * B_1 = (3 f^3 - 6 f^2 + 4) / 6, B_2 = (-3 f^3 + 3 f^2 + 3 f + 1) / 6, B_3 = f^3 / 6; at least
 * floor((n - 1) t_host[a]) + 4 control points per axis (checked).  (x', y', z') is the destination index with the axes of
 * mirror_mask (bit 0 = x, 1 = y, 2 = z) reversed, n - 1 - i: pass the mirrored affine map (image_tools.mirror_index_affine)
 * and the mask, and the result is the flip of the un-mirrored deformed crop.  A rotation is part of M.  The field is
 * evaluated in double; inside test, interpolation and padding are those of the affine entries, a zero control grid gives
 * their result bit for bit, and channel m of the _mc entry equals its M = 1 case -- seg3d_resample_deform -- on plane m
 * bit for bit.  Per-axis
 * weights and the control grid are staged in LDS (at most 64 KB: crop-sized grids). */
int seg3d_resample_deform(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                          const double* affine_host, int linear, float pad, const double* l_host, const float* ctrl,
                          int gx, int gy, int gz, const double* t_host, int mirror_mask, void* stream);
int seg3d_resample_deform_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi, int Xo,
                             int Yo, int Zo, const double* affine_host, int linear, float pad, const double* l_host,
                             const float* ctrl, int gx, int gy, int gz, const double* t_host, int mirror_mask,
                             void* stream);
/* ---- typed sources (compact resident training cases) -------------------------------------
 * seg3d_resample_affine_mc / seg3d_resample_deform_mc for a source kept in the element type of its file: src_dtype is
 * 0 int8, 1 uint8, 2 int16 or 4 float32; code 3 (int32, not exact in a float) and any other value set an error text and
 * return SEG3D_ERR_UNSUPPORTED.  Every element read is converted with (float), which is exact for the four types, and
 * everything after the load is the float entries' arithmetic: the result equals theirs on the converted volume bit for bit,
 * and src_dtype = 4 IS the float entry.  dst is fp32.  Rows of 2-byte elements move as one 8- / 4-byte access at
 * M = 4 / 2 when src is aligned to them (and dst as for the float entries); 1-byte elements take scalar loads.  The B-spline
 * entries have no typed form: they read coefficients. */
int seg3d_resample_affine_typed_mc(const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi, int Yi,
                                   int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                                   void* stream);
int seg3d_resample_deform_typed_mc(const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi, int Yi,
                                   int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                                   const double* l_host, const float* ctrl, int gx, int gy, int gz, const double* t_host,
                                   int mirror_mask, void* stream);
/* ---- cubic B-spline interpolation (not in the reference) ----------------------------------
 * The third interpolation of the resampler, exact: the interpolant passes through the samples.  DEFINITION (stated here
 * and in DESIGN.md, nowhere else):
 *   coefficients  per axis of n voxels the coefficients c of the samples s solve s[i] = (c[i-1] + 4 c[i] + c[i+1]) / 6 with
 *                 indices outside 0 .. n-1 mirrored about the end samples (whole-sample mirror: -1 -> 1, n -> n - 2, in
 *                 general period 2 (n - 1)); n = 1: c = s.  The 3-D coefficients are the three axes applied in turn
 *                 (scipy.ndimage.spline_filter(order = 3, mode = 'mirror')).
 *   recursion     z = sqrt(3) - 2:  c+[0] = sum_{k < 24} z^k s[mirror(k)],  c+[i] = s[i] + z c+[i-1],
 *                 c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),  c-[i] = z (c-[i+1] - c+[i]),  c = 6 c-.  Running values in
 *                 double; c+ and c are stored as fp32.
 *   evaluation    at the continuous index (cx, cy, cz): per axis k = floor(c), f = c - k, taps k-1 .. k+2 with the same
 *                 mirror, weights the uniform cubic basis B_0 .. B_3(f) written out above for the elastic field.  Double,
 *                 one fixed order -- per (z, y) row the x taps k-1 .. k+2 added left to right, then the four rows with the
 *                 y weights, then the four planes with the z weights -- rounded to float once (the convention of the
 *                 trilinear branch).  Inside test and padding are those of seg3d_resample_affine: -0.5 <= c < size - 0.5,
 *                 else `pad`.  Overshoot is not clamped (neither nnU-Net nor ITK clamp).
 * seg3d_bspline_prefilter_mc: samples src [Z][Y][X][M] fp32 (M = 1..8) -> coefficients dst of the same shape; dst == src
 * (in place) or disjoint; any axis length >= 1, 64-bit indexing.  Three passes (x, y, z; an axis of one voxel has none), no
 * workspace, no atomics, no host sync: two runs are bit-equal, channel m equals the M = 1 call on plane m bit for bit,
 * and in place equals out of place bit for bit. */
int seg3d_bspline_prefilter_mc(const float* src, float* dst, int X, int Y, int Z, int M, void* stream);
/* The resampling entries with the spline: arguments and geometry of seg3d_resample_affine(_mc) / seg3d_resample_deform(_mc)
 * without `linear` (index map, inside test, elastic field, mirror mask, dst_stride and padding are theirs), src holds the
 * COEFFICIENTS of seg3d_bspline_prefilter_mc.  A zero control grid gives the affine entry's result bit for bit; channel m
 * of an _mc entry equals its M = 1, dst_stride = 1 case -- the entry without _mc -- on plane m bit for bit. */
int seg3d_resample_bspline(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                           const double* affine_host, float pad, void* stream);
int seg3d_resample_bspline_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi, int Xo,
                              int Yo, int Zo, const double* affine_host, float pad, void* stream);
int seg3d_resample_bspline_deform(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                  const double* affine_host, float pad, const double* l_host, const float* ctrl, int gx,
                                  int gy, int gz, const double* t_host, int mirror_mask, void* stream);
int seg3d_resample_bspline_deform_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi,
                                     int Xo, int Yo, int Zo, const double* affine_host, float pad, const double* l_host,
                                     const float* ctrl, int gx, int gy, int gz, const double* t_host, int mirror_mask,
                                     void* stream);
/* ---- per-label trilinear vote for label maps, 'LABEL_LINEAR' (not in the reference) -------
 * The fourth interpolation of the resampler, for LABEL MAPS only (one channel).  DEFINITION (stated here and in DESIGN.md,
 * nowhere else).  For an output voxel with the continuous source index c:
 *   1. c is the resampler's own: the affine map M (x, y, z, 1), with the elastic field, rotation and mirror handling of
 *      seg3d_resample_deform in the _deform entry.
 *   2. c outside the buffer (not -0.5 <= c < size - 0.5 on every axis): the result is `pad`.
 *   3. Otherwise the eight clamped taps and the weights (dx, dy, dz) are those of the linear branch.
 *   4. For every distinct value l among the eight taps -- compared after the exact (float) conversion of the source element
 *      -- the membership s_l is the linear branch's interpolation (double, order x, y, z, rounded to float once) of the
 *      indicator taps (tap == l ? 1.0 : 0.0).
 *   5. The voxel gets the l with the largest s_l; among equal s_l the smallest l wins.
 *   6. The result is written as a float, as the nearest-neighbour mask crop is.
 * Equivalence: for the labels l of the volume in ascending order (with `pad` added in its sorted place when it is not one of
 * them) let plane_l = seg3d_resample_affine((src == l) as 0 / 1 floats, linear = 1, pad = (l == pad ? 1 : 0)); the result
 * equals the first-maximum arg-max over the planes bit for bit, voxel for voxel (a label that is not among the taps has
 * s_l = 0 and cannot win).  Eight equal taps give that value exactly (1 + (1 - 1) d = 1), without a lerp.  Labels are copied,
 * not interpreted: an ignore label (255) or an out-of-range id votes like any other value.  It is an ARG-MAX, not a
 * threshold: unlike a sequential `>= 0.5` overwrite per label, a voxel where no label reaches 0.5 still gets its strongest
 * label.  src [Zi][Yi][Xi] contiguous of src_dtype 0 int8, 1 uint8, 2 int16 or 4 float32 (finite values); code 3 and unknown
 * codes return SEG3D_ERR_UNSUPPORTED as the typed entries do.  One launch of one thread per output voxel, no workspace, no
 * atomics, 64-bit indexing: two runs are bit-equal.  A zero control grid gives the affine entry's result bit for bit. */
int seg3d_resample_label(const void* src, int src_dtype, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                         const double* affine_host, float pad, void* stream);
int seg3d_resample_label_deform(const void* src, int src_dtype, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                const double* affine_host, float pad, const double* l_host, const float* ctrl, int gx,
                                int gy, int gz, const double* t_host, int mirror_mask, void* stream);
/* Intensity augmentation of a normalised crop [Z][Y][X][M] (M = 1..8, channels-last; M = 1 is the planar crop), IN PLACE.
 * Per modality m, with (mn, mx, mean) of the crop's channel m (min / max exact, mean from an fp64 sum in a fixed order):
 *   brightness  y = x * brightness
 *   contrast    y = clamp(mean + contrast * (y - mean), mn, mx)     (statistics after the brightness step)
 *   gamma       [lo, hi] = the range after the contrast step; hi - lo >= 1e-7: r = (y - lo) / (hi - lo), r = 1 - r if
 *               invert, r = r^gamma, r = 1 - r if invert, y = lo + r (hi - lo); otherwise unchanged
 *   noise       y += sigma * n, n = sqrt(-2 ln u1) cos(2 pi u2), u1 = (r0 + 1) 2^-32, u2 = r1 2^-32, (r0, r1) the first two
 *               outputs of Philox4x32-10 with key (seed_lo, seed_hi) and counter (v_lo, v_hi, m, 0), v = (z Y + y) X + x
 * brightness, contrast, gamma > 0, sigma >= 0 (checked); a neutral parameter (1, 1, 1, 0) skips its step exactly, the two
 * statistics launches run only when some modality has contrast or gamma on, and nothing is launched when all is
 * neutral.  workspace: seg3d_augment_intensity_workspace_doubles doubles (may be NULL without contrast / gamma).
 * grid_blocks: workgroups of the apply pass, 0 = default; the result does not depend on it.  No atomics, no allocation,
 * no host sync: two runs are bit-equal and the call is capturable. */
typedef struct Seg3dIntensity {
  float brightness, contrast, gamma;
  int invert;
  float sigma;
} Seg3dIntensity;
typedef struct Seg3dIntensityParams {
  Seg3dIntensity m[8];
  unsigned int seed_lo, seed_hi;
} Seg3dIntensityParams;
long long seg3d_augment_intensity_workspace_doubles(int X, int Y, int Z, int M);
int seg3d_augment_intensity(float* crop, double* workspace, int X, int Y, int Z, int M, Seg3dIntensityParams params,
                            int grid_blocks, void* stream);
/* Gaussian blur and low-resolution simulation of a normalised crop [Z][Y][X][M] (M = 1..8, channels-last; M = 1 is the
 * planar crop), OUT OF PLACE src -> dst, buffers must not overlap (csrc/augment_filter.hip).
 * One launch for all modalities; no allocation, no host sync, no atomics: two runs are bit-equal and the calls are
 * capturable.  A voxel's value is a function of the crop and the parameters alone (not of tiling, M or alignment).
 *   blur    per modality m: radius[m] = R in 0..6 and the 2R + 1 taps w[-R..R] in taps[m][0..R] (taps[m][k] = w[+-k], the
 *           host computes them in double: exp(-k^2 / (2 s^2)) normalised over -R..R).  Separable x, then y, then z, fp32,
 *           taps added in the order -R..R, no FMA contraction.  Border: half-sample reflection (d c b a | a b c d | d c b a),
 *           i' = i mod 2n, i' >= n -> 2n - 1 - i', valid for any n and R.  radius[m] = 0 copies the modality bit for bit.
 *   lowres  per modality the low-grid sizes 1 <= n' <= n of the three axes.  Down-sampling is nearest, centre-aligned:
 *           low voxel j takes source voxel s(j) = min(n - 1, ((2 j + 1) n) / (2 n')).  Up-sampling is Keys cubic convolution
 *           (a = -0.5), separable: t = (2 i + 1) n' - n, k = floor(t / 2n), f = (t - 2 n k) / 2n, output voxel i takes the low
 *           voxels k-1 .. k+2 clamped to [0, n' - 1] with the weights -0.5 f^3 + f^2 - 0.5 f, 1.5 f^3 - 2.5 f^2 + 1,
 *           -1.5 f^3 + 2 f^2 + 0.5 f, 0.5 f^3 - 0.5 f^2; x innermost, then y, then z, taps added in the order k-1 .. k+2.
 *           The low grid is never stored.  An axis with n' = n has weights (0, 1, 0, 0); all three equal: bit-exact copy.
 * When every modality is off, one copy kernel is launched. */
typedef struct Seg3dBlurParams {
  int radius[8];
  float taps[8][7];
} Seg3dBlurParams;
typedef struct Seg3dLowresParams {
  int nx[8], ny[8], nz[8];
} Seg3dLowresParams;
int seg3d_augment_blur(const float* src, float* dst, int X, int Y, int Z, int M, Seg3dBlurParams params, void* stream);
int seg3d_augment_lowres(const float* src, float* dst, int X, int Y, int Z, int M, Seg3dLowresParams params, void* stream);
/* box_device[6] initialised to {INT_MAX x3, -1 x3} -> inclusive (xmin, ymin, zmin, xmax, ymax, zmax) of the voxels whose
 * value is in labels_host (nlabels == 0: every voxel > 0); untouched when nothing is selected */
int seg3d_mask_bounding_box(const signed char* mask, int X, int Y, int Z, const int* labels_host, int nlabels,
                            int* box_device, void* stream);
/* 26-connected components of (mask == label): keep the largest (mode 0; ties: first in raster order) or every component
 * with >= threshold voxels (mode 1); out = (combine ? out : 0) + value * kept.  workspace: seg3d_ccl_workspace_ints ints */
long long seg3d_ccl_workspace_ints(long long voxels);
int seg3d_ccl26_select(const signed char* mask, int label, int X, int Y, int Z, int mode, int threshold, int value,
                       int combine, signed char* out, int* workspace, void* stream);

/* ---- lesion-wise evaluation (not in the reference; csrc/lesion.hip, csrc/postproc.hip) -----
 * Building blocks of lesion-wise Dice / HD95: the ground truth of a target (a set of label ids) is dilated by the
 * 18-neighbourhood and split into 26-connected lesions, the prediction into 26-connected components, and every
 * (lesion, component) pair that shares a voxel is recorded.  Volumes are [Z][Y][X] with fewer than 2^31 voxels.  Integer
 * work with integer atomics only: every result is exact and identical from run to run.  No entry allocates or
 * synchronises, no workgroup waits on another, and every loop has a bound known at launch (capturable).
 *
 * seg3d_label_set_mask: mask[i] = 1 iff labels[i] is an integer l in [0, 256) with bit (l & 31) of set.bits[l >> 5]
 * set, else 0.  dtype codes as seg3d_label_overlap_counts.
 *
 * seg3d_binary_dilate18: out = mask dilated `iters` times (0..16) by the 18-neighbourhood: a voxel is set if it, or a
 * neighbour differing by +-1 in at most two axes, was set; nothing exists outside the volume.  One launch per iteration,
 * ping-ponging between out and workspace (X*Y*Z bytes, needed for iters >= 2) so that the last lands in out; iters = 0
 * copies.  mask, out and workspace must be distinct.
 *
 * seg3d_ccl26_label: ids[v] = 0 where mask[v] == 0, else the id 1..K of v's 26-connected component, ids in the order
 * of each component's lowest linear voxel index (z*Y + y)*X + x -- independent of the launch order.  count_device[0] = K,
 * count_device[1] = 1 iff K > capacity (an ordinary return: repeat with a larger sizes array), else 0.  sizes[k - 1] =
 * voxels of component k for k <= capacity; nothing is written at or beyond sizes[capacity].  workspace:
 * seg3d_ccl26_label_workspace_ints ints (-1: bad size).
 *
 * seg3d_lesion_pairs: one pass over dmap (lesion ids 0..kg), a (0/1 ground-truth mask) and pmap (component ids, 0 =
 * none).  gsize[i] += |{v : dmap = i, a}|, inter[i] += |{v : dmap = i, a, pmap > 0}| (int64, kg + 1 entries each, zeroed
 * by the caller), and every distinct key (i << 32 | j) with dmap = i > 0, pmap = j > 0 is inserted into table, an
 * open-addressing hash set of `capacity` (a power of two) 64-bit words zeroed by the caller (0 = empty; linear probing,
 * at most capacity probes).  A key that finds no slot sets status[0] (zeroed by the caller) to 1 and nothing else is
 * lost: the counts are complete, and the caller repeats the launch with a larger table.  collapse != 0: lanes of a wave
 * with equal keys are merged before the atomics (the default of the Python wrapper); 0: one set of atomics per voxel.
 * The results do not depend on it.
 *
 * seg3d_lesion_select: g[v] = (dmap[v] == lesion && a[v]), u[v] = flag[pmap[v]] != 0 (flag: kp + 1 device bytes, pmap
 * outside 1..kp gives 0), both as 0/1 bytes: label 1 of a uint8 volume for seg3d_label_surface.  Whole volume. */
typedef struct Seg3dLabelSet {
  unsigned int bits[8];
} Seg3dLabelSet;
int seg3d_label_set_mask(const void* labels, int dtype, long long n, Seg3dLabelSet set, unsigned char* mask, void* stream);
int seg3d_binary_dilate18(const unsigned char* mask, unsigned char* out, unsigned char* workspace, int X, int Y, int Z,
                          int iters, void* stream);
long long seg3d_ccl26_label_workspace_ints(long long voxels);
int seg3d_ccl26_label(const unsigned char* mask, int X, int Y, int Z, int* ids, int* count_device, int* sizes, int capacity,
                      int* workspace, void* stream);
int seg3d_lesion_pairs(const int* dmap, const unsigned char* a, const int* pmap, long long n, int kg, long long* gsize,
                       long long* inter, unsigned long long* table, long long capacity, int collapse, int* status,
                       void* stream);
int seg3d_lesion_select(const int* dmap, const unsigned char* a, const int* pmap, const unsigned char* flag, int kp,
                        int lesion, long long n, unsigned char* g, unsigned char* u, void* stream);

/* ---- whole-volume statistics for case-level normalisation (not in the reference; DESIGN.md section 7 row f20;
 * csrc/volume_stats.hip) --------------------------------------------------------------------------------------------------
 * volume: fp32 channels-last [Z][Y][X][M], 1 <= M <= 8, `voxels` = Z*Y*X in [1, 2^31); sel: uint8 [Z][Y][X] or NULL.
 * Selection set S_m of modality m:  mode 0 = every voxel;  mode 1 = x != 0, decided on the bits (-0.0 is out, a denormal
 * is in);  mode 2 = sel[v] != 0, the same set for every m.
 * Per modality, out[m][9] (device doubles) = n, min, max, mean, std, value(q_0) .. value(q_3):
 *   n = |S_m|; min / max of S_m; -0.0 is reported as +0.0 everywhere;
 *   value(q) = sorted(S_m)[k], k = floor(q (n - 1) + 0.5) computed in double on the device from the device's n, q in
 *     [0, 1], Q <= 4 of them (entries past Q are 0).  This is the NEAREST RANK: it differs from the linearly interpolated
 *     percentile (numpy's default) by less than the gap between two neighbouring order statistics;
 *   mean and population std in fp64 of S_m, std floored at 1e-6; with clip != 0 (needs Q >= 2, q_0 <= q_1) of the values
 *     clamped to [value(q_0), value(q_1)] (the CT rule);
 *   n == 0: every output is 0 and std is the floor.
 * The order statistics come from a three-level radix select (11 / 11 / 10 bits) over the order-preserving integer key of
 * the float; n, min, max and the order statistics are exact, and with integer atomics only and a fixed-order fp64 sum of
 * per-workgroup partials two runs are bit-equal in every output.  NaN / Inf are outside the value contract (the kernels
 * stay inside their buffers and terminate).
 * Split entries, so that histograms and moments can be accumulated over several volumes (a data set) before they are
 * resolved; every volume must be passed to every level with the same M, mode and sel:
 *   seg3d_volume_stats_begin                      zero the state
 *   for level in 0, 1, 2 (level 0 alone when Q == 0):
 *     seg3d_volume_stats_accumulate_hist          once per volume: this level's digit histograms (and min / max at level 0)
 *     seg3d_volume_stats_resolve                  once: level 0 derives n and the ranks (equal ranks are resolved once);
 *                                                 each level fixes its digit of every rank's key
 *   seg3d_volume_stats_accumulate_moments         once per volume (after the resolves: the clamp and the pivot of the
 *                                                 sums come from the state)
 *   seg3d_volume_stats_finish                     out[m][9]
 * seg3d_volume_stats is that sequence for one volume.  quantiles: Q doubles in HOST memory.  state:
 * seg3d_volume_stats_state_bytes(M) bytes of device memory, 8-byte aligned (0: bad M); layout: control block (8 x 32
 * int64: n, min key, max key, and per rank k, key prefix, rank inside the chosen bin, alias), level-0 histograms [M][2048],
 * level-1 [M][4][2048], level-2 [M][4][1024] (all uint64), moment slots [2048][M][2] doubles.  No entry allocates, reads
 * back or synchronises, nothing data-dependent is baked into a launch (capturable).  Rows of M floats are read as one
 * 16- / 8-byte load when M is 4 / 2 and the volume is so aligned, else by scalar loads; the results do not depend on it. */
long long seg3d_volume_stats_state_bytes(int M);
int seg3d_volume_stats_begin(void* state, int M, void* stream);
int seg3d_volume_stats_accumulate_hist(const float* volume, const unsigned char* sel, long long voxels, int M, int mode,
                                       int level, void* state, void* stream);
int seg3d_volume_stats_resolve(void* state, int M, int Q, const double* quantiles, int level, void* stream);
int seg3d_volume_stats_accumulate_moments(const float* volume, const unsigned char* sel, long long voxels, int M, int mode,
                                          int clip, void* state, void* stream);
int seg3d_volume_stats_finish(void* state, int M, int Q, int clip, double* out, void* stream);
int seg3d_volume_stats(const float* volume, const unsigned char* sel, long long voxels, int M, int mode, int Q,
                       const double* quantiles, int clip, void* state, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEG3D_HIP_H */
