/*
 * forge_hip.h — C-ABI of libforge_hip.so, the MI355X (gfx950) kernels behind the FORGE
 * reconstruction hot path (UT-Austin-RPL/FORGE: models/rotate.py, models/volume_render.py,
 * models/fusion.py, models/encoder.py).
 *
 * The reference is pure Python/PyTorch (no FFI of its own); the drop-in boundary for callers is
 * the Python nn.Module surface in forge_amd/ (same class/method/state_dict names as
 * models/model.py etc.).  This header is the boundary ONE level lower: what forge_amd's host
 * code (or any other host language) binds.  Each entry point cites the
 * reference call site it replaces.
 *
 * Conventions
 *   - plain C types only: device pointers (const float*), ints, floats, an opaque stream handle
 *     (hipStream_t passed as void*; NULL = the default stream).  No torch types.
 *   - every function returns 0 on success, a positive hipError_t when a HIP call failed, or a
 *     negative FORGE_E* code for a rejected argument; forge_last_error() gives the message
 *     (thread-local).
 *   - functions are re-entrant, allocate nothing and keep no global state: all buffers
 *     (including workspaces) are owned by the caller.
 *   - launches are asynchronous on `stream`; nothing synchronises.
 *   - volumes are CHANNELS-LAST fp32: vol[n][D][H][W][C] (torch: an NCDHW tensor in
 *     torch.channels_last_3d memory format); grid axes (x,y,z) <-> tensor axes (W,H,D)
 *     exactly as in F.grid_sample / pytorch3d Volumes.
 */
#ifndef FORGE_HIP_H
#define FORGE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* forge_stream_t; /* hipStream_t */

#define FORGE_EINVAL (-1)   /* bad argument value (null pointer, non-positive dim, ...) */
#define FORGE_ESHAPE (-2)   /* unsupported shape (e.g. C not a multiple of 4)            */

/* Library version: major*10000 + minor*100 + patch. */
int forge_version(void);
/* Message for the last non-zero return on this thread ("" if none). */
const char* forge_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * a2  voxel-grid pose warp — replaces models/rotate.py:127-141 (affine grid + F.grid_sample
 * trilinear, zeros padding, align_corners=FALSE, then cat with view 0).
 *
 *   vox  [n][D][H][W][C]   input volumes (all views of all scenes, n = B*t)
 *   xf   [n][12]           row-major 3x4 affine in NORMALISED grid coords: for the output voxel
 *                          with g = (gx,gy,gz), g_a = 2 i_a/(N_a-1) - 1, the sample coordinate is
 *                          s = A g + b  (A = R_T, b = t_T / grid_coord_max; rotate.py:132-135)
 *   mode [n]               0: copy the volume unchanged (view 0, rotate.py:141); 1: warp
 *   out  [n][D][H][W][C]
 * pixel coord p_a = ((s_a+1) N_a - 1)/2 (align_corners=False), 8 taps each zeroed when out of range.
 * Requires C % 4 == 0.
 */
int forge_rotate_fwd(const float* vox, const float* xf, const int* mode, float* out,
                     int n, int C, int D, int H, int W, forge_stream_t stream);

/* forge_rotate_fwd with the view ordering of models/model.py:127-128 (`chose_selected(features_transformed, idxs)`) fused into the
 * store: input volume i is written to output volume dst_slot[i] (a permutation of 0..n-1 on the device) instead of i - saves the
 * gather copy of all warped volumes (84 MB read + written per 5-view scene). Inference only (no backward counterpart). */
int forge_rotate_fwd_slots(const float* vox, const float* xf, const int* mode, const int* dst_slot, float* out,
                           int n, int C, int D, int H, int W, forge_stream_t stream);

/* models/rotate.py:64-89,132-135 on the device: poses [B][t][4][4] (row-major camera poses, view 0 = reference) ->
 * xf [B*t][12] = [R_T | t_T / half_extent] with T = P_0 P_i^-1 (general 4x4 inverse), mode [B*t] = (0,1,1,...).
 * Feeds forge_rotate_fwd without any host round trip. (Gradients w.r.t. poses go through the host-side torch
 * algebra instead, see forge_amd/rotate.py.)
 * slot (nullable) [B*t]: the view order of models/model.py:152-158 (`sequence_from_distance`: views sorted by squared distance of their
 * camera position to view 0's, ties by view index = a stable sort) as the dst_slot array of forge_rotate_fwd_slots:
 * slot[b t + i] = b t + rank of view i. dist (nullable) [B*t]: the sort keys, when the caller wants its own distance values ranked
 * (the torch host passes sequence_from_distance's: symmetric camera rigs produce near-ties whose order must not depend on who
 * rounded the sum of squares); NULL: computed here as ((dx^2 + dy^2) + dz^2) without fused multiply-adds.
 */
int forge_rotate_xf_from_poses(const float* poses, float* xf, int* mode, int* slot, const float* dist, int B, int t, float half_extent,
                               forge_stream_t stream);

/* Pose chain of the refinement loop (kubric_eval.py:412-530 `do_refinement`, demo.py:115-188): from the optimised relative poses of the
 * non-reference views - rot [b (t-1)][4] raw quaternions (w, x, y, z; normalised here as F.normalize + utils/geo_utils.py:122-137 do),
 * trans [b (t-1)][3] - to both kernel operands in one launch:
 *   poses [b t][16]  canonical_pose @ [R(q) | trans] (view 0: canonical_pose itself)            utils/geo_utils.py:268-287
 *   xf [b t][12], mode [b t]   the warp's affine [R_T | t_T / half_extent], T = P_0 P_i^-1       models/rotate.py:64-89,132-135
 *   slot [b t]       (nullable) the view order of models/model.py:152-158 as forge_rotate_fwd_slots' dst_slot (see forge_rotate_xf_from_poses)
 *   cam16 [b t][16]  the ray-marcher's cameras [R | T | fx fy cx cy] from the extrinsics P_i^-1 and K / 2   models/volume_render.py:40-51
 *   origin [b t][2]  (nullable) projection of the world origin (models/volume_render.py:77-79)
 *   jac [b (t-1)][24][7] (nullable) d(xf[0..11], cam16[0..11]) / d(quaternion, translation), by forward-mode differentiation in the kernel
 * can_pose / can_extr: row-major 4x4 pose / extrinsics of the reference view; K [b t][9] full-resolution intrinsics.
 * forge_pose_chain_bwd: drot [b (t-1)][4], dtrans [b (t-1)][3] = jac^T (dxf row | dcam row[0..11]) (dxf [b t][12] from forge_rotate_bwd,
 * dcam [b t][16] from forge_render_bwd; either nullable). Replaces ~250 torch launches of 3-8 us per refinement iteration. */
int forge_pose_chain_fwd(const float* rot, const float* trans, const float* can_pose, const float* can_extr, const float* K, float half_extent,
                         int b, int t, float* xf, int* mode, int* slot, float* cam16, float* poses, float* origin, float* jac, forge_stream_t stream);
int forge_pose_chain_bwd(const float* jac, const float* dxf, const float* dcam, float* drot, float* dtrans, int b, int t, forge_stream_t stream);

/* Backward of forge_rotate_fwd w.r.t. the volumes (and optionally the affine).
 *   dout [n][D][H][W][C]   upstream gradient
 *   dvox [n][D][H][W][C]   nullable (frozen volumes: pose refinement wants dxf only); written (not accumulated): the exact transpose of
 *                          the warp, computed as a gather per source voxel (deterministic, no atomics); mode 0 volumes: plain copy of dout
 *   dxf  [n][12]           nullable; MUST be zero-filled; d loss / d xf (pose refinement,
 *                          kubric_eval.py:469-503). Needs vox (nullable when dxf is NULL).
 */
int forge_rotate_bwd(const float* dout, const float* vox, const float* xf, const int* mode,
                     float* dvox, float* dxf, int n, int C, int D, int H, int W,
                     forge_stream_t stream);
/* The same for a forward that stored view i at volume slot[i] (forge_rotate_fwd_slots): view i's upstream gradient is read at dout[slot[i]]. */
int forge_rotate_bwd_slots(const float* dout, const float* vox, const float* xf, const int* mode, const int* src_slot,
                           float* dvox, float* dxf, int n, int C, int D, int H, int W, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a6  fused ray sampler + volume sampler + emission-absorption ray-marcher — replaces
 * models/volume_render.py:53-63 (cameras_from_opencv_projection, NDCGridRaysampler,
 * VolumeRenderer/VolumeSampler with align_corners=TRUE trilinear zero-pad sampling,
 * EmissionAbsorptionRaymarcher incl. the README.md:26-33 depth patch).
 *
 *   feat     [nvol][D][H][W][C]   render features, channels-last, C % 4 == 0, C <= 32
 *   dens     [nvol][D][H][W]      densities (>= 0, NOT clamped <= 1: models/model.py:140-141)
 *   cam      [V][16]              per view: R[9] row-major (OpenCV world->cam), T[3], fx, fy, cx, cy
 *                                 of the HALF-resolution intrinsics (volume_render.py:50-51)
 *   view2vol [V]                  volume index rendered by each view (replaces the V-fold
 *                                 `repeat` of the volumes, models/model.py:138-139)
 *   out_feat [V][Hr][Wr][C]       sum_s w_s f_s           (channels-last, what the conv_rgb GEMM consumes)
 *   out_opac [V][Hr][Wr]          1 - prod_s (1 - d_s)
 *   out_depth[V][Hr][Wr]          sum_s w_s z_s, nullable (render_depth=False)
 * Ray (h,w): d_cam = ((w+.5-cx)/fx, (h+.5-cy)/fy, 1); p_s = -R^T T + R^T d_cam z_s,
 * z_s = zmin + s (zmax-zmin)/(S-1); local = p / (hx,hy,hz); pix = (local+1)/2 (N-1).
 */
int forge_render_fwd(const float* feat, const float* dens, const float* cam, const int* view2vol,
                     float* out_feat, float* out_opac, float* out_depth,
                     int V, int nvol, int C, int D, int H, int W, int Hr, int Wr, int S,
                     float zmin, float zmax, float hx, float hy, float hz,
                     forge_stream_t stream);

/* Camera dict of models/volume_render.py:40-51 ({'R' [V,3,3], 'T' [V,3], 'K' [V,3,3]}, element strides given: the tensors are usually
 * slices of [V,4,4] extrinsics) -> cam [V][16] as forge_render_fwd takes it, with the reference's half-resolution intrinsics
 * (K / 2, K[2][2] = 1, on a copy), and (origin nullable) the screen projection of the world origin of :77-79,
 * (fx tx / tz + cx, fy ty / tz + cy). One launch instead of a dozen tensor ops per forward; inference only (the differentiable form
 * for camera gradients is host-side torch algebra, forge_amd/volume_render.py). */
int forge_pack_cameras(const float* R, long long r0, long long r1, long long r2, const float* T, long long t0, long long t1,
                       const float* K, long long k0, long long k1, long long k2, float* cam16, float* origin, int V, forge_stream_t stream);

/* Backward of forge_render_fwd w.r.t. volumes (and optionally cameras) - what autograd through PyTorch3D's VolumeSampler /
 * EmissionAbsorptionRaymarcher computes for models/volume_render.py:63. Deterministic (no atomics): a ray-parallel pass leaves the two
 * per-sample scalars (dL/dd_s, T_s d_s) in the workspace, a voxel-parallel gather sums every voxel's tap contributions in a fixed order.
 *   g_feat [V][Hr][Wr][C], g_opac [V][Hr][Wr], g_depth [V][Hr][Wr] (nullable)
 *   dfeat  [nvol][D][H][W][C], ddens [nvol][D][H][W]   WRITTEN (every element; no zero-fill needed, nothing accumulated)
 *   dcam   [V][16] nullable, WRITTEN: d loss / d (R, T, fx, fy, cx, cy)
 *   ws     caller-owned scratch of at least forge_render_bwd_ws_bytes(V, C, Hr, Wr, S, dcam != NULL) bytes, 16-byte aligned
 *          (8 V Hr Wr S bytes; when dcam is requested + 64 bytes per 8 x (64 / (C/4)) pixel tile and view + 24 V Hr Wr S bytes of per-sample
 *          position-gradient scalars that the ray pass's forward march leaves for its own backward sweep); no allocation inside.
 */
long long forge_render_bwd_ws_bytes(int V, int C, int Hr, int Wr, int S, int want_cam);     /* < 0: unsupported arguments */
int forge_render_bwd(const float* feat, const float* dens, const float* cam, const int* view2vol,
                     const float* g_feat, const float* g_opac, const float* g_depth,
                     float* dfeat, float* ddens, float* dcam,
                     int V, int nvol, int C, int D, int H, int W, int Hr, int Wr, int S,
                     float zmin, float zmax, float hx, float hy, float hz,
                     void* ws, long long ws_bytes, forge_stream_t stream);

/* a7  mask / depth up-sampling (models/volume_render.py:69,74: F.upsample(size=img_size, mode='bilinear') = align_corners False): P planes
 * [Hi][Wi] -> [Ho][Wo] with ATen's source-index / weight arithmetic; _bwd is the adjoint (a deterministic gather per input pixel, written). */
int forge_resize_bilinear_fwd(const float* in, float* out, int P, int Hi, int Wi, int Ho, int Wo, forge_stream_t stream);
int forge_resize_bilinear_bwd(const float* g, float* din, int P, int Hi, int Wi, int Ho, int Wo, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a1/a4/a5  implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32)
 * with fused element-wise tails — replaces the cuDNN convolutions + separate element-wise ops of
 * models/fusion.py:29-35 (ConvGRU cell: cat, conv, split, sigmoid, mul, cat, conv, tanh, lerp),
 * models/fusion.py:61-68 (fusion_conv), models/encoder.py:36-40 (conv1) and :16-34 (heads; the
 * ConvTranspose3d k4 s2 p1 runs as 8 output-phase GEMMs of 8 taps each).
 *
 *   rows                        the GEMM rows enumerate an (n,D,H,W) grid, M = n D H W
 *   in1 / in2                   channels-last inputs on an (n,Di,Hi,Wi) grid; row of GEMM-grid voxel
 *                               (z,y,x) and tap (dz,dy,dx) is input voxel (z is+dz, y is+dy, x is+dx),
 *                               zero outside the grid. The conv sees C1 channels of in1 followed by C2 of
 *                               in2 (in2 NULL <=> C2 = 0); ld1/ld2 = row strides in floats (>= C1/C2, so a
 *                               channel slice of a wider tensor can be fed). C1, C2 % 32 == 0. bs1/bs2 = batch
 *                               strides in rows (0 = dense Di Hi Wi): lets view t of a [b][t] stack be fed in place.
 *   wp  [ntaps][Cout][C1+C2]    packed weights: wp[t][co][ci] multiplies in[voxel + taps[t]][ci]
 *   taps [ntaps][3]             HOST array of (dz,dy,dx) input offsets, ntaps <= 27, every component in [-128, 127] (FORGE_EINVAL
 *                               otherwise: the kernels carry taps as signed bytes)
 *   out rows                    output voxel of GEMM-grid voxel (z,y,x) is (z os+pz, y os+py, x os+px)
 *                               in an (n,Do,Ho,Wo) grid; row stride ldo floats.
 *                               plain conv: is=os=1, Di=Do=D..; strided conv: is=2; ConvTranspose phase: os=2.
 *                               pz = py = px = -1 with os = 2: ALL output phases of a stride-2 transposed convolution in one
 *                               launch - taps / wp hold the phases back to back (8 phases for Do = 2D, 4 for a 2-D grid with
 *                               Do = D; phase p = pz*4 + py*2 + px uses taps [p*ntaps/P, (p+1)*ntaps/P)); no split-K.
 *   epilogue 0  out = acc + bias
 *            1  out = lrelu((acc + bias) * scale + shift + residual, slope)   eval-BN folded; residual
 *               [rows][ldo] nullable (ResNet shortcut); slope 1 = identity, 0 = ReLU. residual may be `out` itself (in place,
 *               element for element); no other overlap of residual and out is allowed (see forge_conv_igemm_epilogue)
 *            2  GRU gates (Cout = 2 Ch): out[m][c] = sigmoid(v_c), c < Ch (update);
 *                                        out2[m][c] = aux_h[m][c] * sigmoid(v_{Ch+c})  (h * reset)
 *            3  GRU state: hn = aux_h (1 - aux_z) + tanh(v) aux_z; out = hn;
 *                          out2 (nullable) = hn * scale + shift          (fusion_norm on the last step)
 *            epilogues 2 / 3 add `residual` [rows][Cout] (nullable) to the pre-activation: the input half conv(x, W_x) of
 *            conv([x, h], W) = conv(x, W_x) + conv(h, W_h), computed once per view when several fusions share views.
 *   out3 (nullable, epilogues 2 / 3 only): what a hand-written backward of the fused cell needs besides out / out2 -
 *            epilogue 2: the reset gate sigmoid(v_{Ch+c}) [M][Ch]; epilogue 3: the candidate tanh(v) [M][Cout]
 *            (pose refinement with frozen weights runs the fused epilogues in forward, forge_amd/fusion.py).
 * bias/scale/shift [Cout]; bias nullable.
 *   lift > 0 (epilogue 1, 2-D conv i.e. D = 1): fuses the 2D->3D feature lift of models/encoder.py:49 into the store —
 *            GEMM column j = z*(Cout/lift) + c of row (n, h, w) is written to out[n][z][h][w][c] (a channels-last
 *            (n, lift, H, W) volume with Cout/lift channels). The caller orders the weight rows accordingly.
 *   tile / ksplit: the launch plan. tile = 0: planned inside the call (forge_conv_igemm_plan's model; split-K only if splitk_ws is given).
 *            tile = 'A'..'E' with ksplit >= 1: the caller's plan, taken verbatim (normally forge_conv_igemm_plan's answer, so that the
 *            caller can size splitk_ws to ksplit M Cout floats; also how tools / tests pin a tile). Ignored for Cout <= 16.
 *   splitk_ws (nullable, splitk_ws_bytes): scratch for split-K. When the M x Cout tile grid alone cannot fill the chip
 *            (< 512 workgroups, e.g. ResNet layers at M = 5120) the tap x channel reduction is sliced over up to 8 workgroups
 *            per tile; raw partial tiles go to splitk_ws[slice][M][Cout] and a second kernel sums them in a fixed order and
 *            applies the epilogue (epilogues 0 and 1 only). NULL disables it. Results are deterministic either way.
 *   stats (nullable; epilogue 0 of the wide kernel, plain output mapping, no split-K): the column sums and sums of squares of the OUTPUT per
 *            32-row block of M, float64, stats[block][2][Cout] for ceil(M / BM) BM / 32 blocks, BM = the tile's rows (128 for tiles A, C, E; 64 for B, D;
 *            every block is written, blocks past M with partial / zero sums) - the
 *            batch statistics of the BatchNorm behind the convolution as a by-product of the epilogue (fixed order, no atomics):
 *            forge_bn_train_fwd / forge_bn_sync_stats take them as their partial sums (nblk_pre) instead of re-reading the activation.
 *            The block count depends on the tile, and a split-K plan skips the epilogue: a call with stats != NULL must pass an explicit
 *            `tile` ('A'..'E', forge_conv_igemm_plan's answer) and ksplit <= 1 - tile = 0 (planned inside) is refused with FORGE_EINVAL.
 *   M = n D H W must be < 2^31.
 */
int forge_conv_igemm(const float* in1, int C1, int ld1, long long bs1, const float* in2, int C2, int ld2, long long bs2,
                     const float* wp,
                     const float* bias, const float* scale, const float* shift, float slope, const float* residual,
                     const float* aux_h, const float* aux_z, float* out, float* out2, float* out3,
                     int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout, int ldo,
                     const int* taps, int ntaps, int os, int pz, int py, int px, int Do, int Ho, int Wo,
                     int epilogue, int lift, int tile, int ksplit, float* splitk_ws, long long splitk_ws_bytes, double* stats, forge_stream_t stream);

/* The launch plan forge_conv_igemm will use for a problem (M = n*D*H*W GEMM rows, Cout, Cin = C1 + C2, ntaps): *tile gets the
 * workgroup tile ('A' 128x128, 'B' 64x128, 'C' 128x64, 'D' 64x64, 'E' 128x32 output rows x channels; 'N' = the Cout <= 16 kernel),
 * *ksplit the number of K-slices (1 = no split-K); nphase = 1, or 4 / 8 for a merged-phase transposed-conv launch (M rows and ntaps / nphase
 * taps per phase). Pure host arithmetic (a makespan model of the 256-CU chip), no launch; lets a
 * caller size the split-K workspace (ksplit * M * Cout floats) and lets profilers attribute launches to kernel instantiations. */
int forge_conv_igemm_plan(long long M, int Cout, int Cin, int ntaps, int nphase, int epilogue, int ldo, long long splitk_ws_bytes,
                          int* tile, int* ksplit);

/* The two epilogues of the wide kernel (Cout > 16) behind forge_conv_igemm and forge_wino_gemm. A launch with identity output rows stores its tile
 * directly through a 32-bit buffer descriptor of the output ("direct-store" epilogue); every other launch maps its rows through a table in LDS (the
 * "general" epilogue). Both store the same bits. The direct-store epilogue reads `residual` ahead of its stores: `residual` may BE `out` (in place,
 * same row stride, element for element: each lane reads exactly what it writes) - any other overlap of the two is not allowed, in either epilogue.
 *   forge_conv_igemm_epilogue: *fast = 1 when a launch takes the direct-store epilogue. That is: the switch below is on, Cout > 16, ksplit == 1,
 *       os == 1 with the output grid equal to the row grid (same_grid) and a single phase (nphase == 1), lift == 0, no stats, epilogue 0 or 1,
 *       Cout <= ldo < 2^22 and ((M - 1) ldo + Cout) 4 < 2^31, and with a residual (epilogue 1) the same two conditions on ldr. Host arithmetic, no launch.
 *   forge_conv_fast_epilogue(on): process-wide switch for A/B measurements and tests, default 1; on = 0 sends every launch through the general
 *       epilogue, on < 0 only queries. Returns the previous setting (0 / 1), never an error. */
int forge_conv_igemm_epilogue(long long M, int Cout, int ldo, int ldr, int has_residual, int os, int same_grid, int nphase, int lift, int ksplit,
                              int has_stats, int epilogue, int* fast);
int forge_conv_fast_epilogue(int on);

/* ---------------------------------------------------------------------------------------------
 * a4 (inference)  the stride-1 3x3x3 convolutions of the ConvGRU fusion (models/fusion.py:29-35, 61-68, 88-95) as Winograd
 * F(2x2, 3x3) over (H, W) with the three depth taps summed directly: 12 instead of 27 multiplies per output and channel pair.
 *   y[z, 2th+i, 2tw+j] = sum_kd A^T [ U[kd] (.) (B^T d[z+kd-1] B) ] A,   U[kd] = G w[kd] G^T,   d = the 4x4 patch at (2th-1.., 2tw-1..)
 * Three launches per convolution, all on channels-last rows, tile rows r = ((n D + z) H/2 + th) W/2 + tw, point p = 4 i + j:
 *   forge_wino_input   V[p][r][c] = (B^T d B)[p] for the C channels of in (rows [n][D][H][W] x ld floats, batch stride bs rows,
 *                      0 = dense); V[p] starts at V + p ptv floats (0 = dense R x ldv), rows of ldv floats. H, W even; C % 4 == 0.
 *   forge_wino_gemm    Mm[p][r][co] = sum_kd sum_ci U[p][kd][co][ci] (V1 | V2)[p][r + kd plane][ci]  for the 16 points in ONE launch of the
 *                      fp32-MFMA implicit-GEMM kernel (forge_conv_igemm's: 3 depth taps over the (n, D, Ht, Wt) tile grid, K = 3 (C1+C2));
 *                      V1 / V2: channel-concatenated operands (V2 nullable with C2 = 0) with row strides ld, batch strides bs rows
 *                      (0 = dense) and point strides pt floats (0 = dense planes of R rows, R ld:
 *                      with a batch stride bs > D Ht Wt the planes are longer than that - pass pt explicitly, here and to forge_wino_wgrad); U [16][kd][Cout][C1+C2]; Mm [16][R][Cout] dense. C1, C2 % 32 == 0,
 *                      Cout > 16. tile: 0 = forge_wino_gemm_tile's rule (Cout <= 64: 'D' below 2048 tile rows, 'C' from there; wider: 'D' / 'B'), or 'A'..'E'.
 *   forge_wino_output  y = A^T (Mm + Mm2) A per tile (row stage first: s = A^T m over i as (m0 + m1) + m2 | (m1 - m2) - m3, then the same over j),
 *                      v = y + bias + residual (residual [rows][Cout] DENSE, nullable, in EVERY epilogue), then the tail on forge_conv_igemm's operands:
 *                        0  out = v                                  1  out = lrelu(v * scale + shift, slope)
 *                        2, 3  forge_conv_igemm's GRU gates / state on the pre-activation v (aux_h / aux_z / out2 / out3 as there)
 *                      Epilogue 1 is NOT forge_conv_igemm's: the residual is added BEFORE the affine map here, after it there; the two agree when
 *                      scale = 1 (how convops.conv3_launch uses the direct kernel) or without a residual.
 *                      ldo: row stride in floats of out (epilogues 0, 1, 3; also of out2 / out3 of epilogue 3), ldo >= Cout and a multiple of 4.
 *                      Epilogue 2 writes out / out2 / out3 as dense rows of Cout / 2 floats and accepts ldo == Cout / 2 only. aux_h / aux_z /
 *                      residual rows are always dense (Cout, or Cout / 2 for the gates' aux_h). FORGE_ESHAPE otherwise.
 *                      Mm2 (nullable): a second set of point products with batch stride bs2 rows and point stride pt2 floats (0 = as Mm) -
 *                      the input half conv(x, W_x) of conv([x, h], W), computed once per view when several fusions share views.
 *   forge_wino_weights U [16][kd][Cout][Cin] = G w[kd] G^T from forge_conv_igemm's packed weights wp [9 kd][Cout][Cin] (float64 inside, rounded
 *                      once); transpose != 0: the weights of the DATA GRADIENT of that convolution instead, U [16][kd][Cin][Cout]
 *                      (dx = the Winograd convolution of dy with them) - a few microseconds, so training re-derives U every step.
 * kd = 3: 3x3x3 kernels (three depth taps summed inside the point GEMMs); kd = 1: the 3x3 kernels of a 2-D convolution (ResNet
 * bottlenecks: the planes of the (n, D) grid do not mix, so images can sit on either axis).
 * B^T and A^T hold 0 / +-1 only (exact additions); U is rounded once from a float64 product. Not bit-identical to
 * forge_conv_igemm (different order of the fp32 additions); measured against a float64 convolution in units of u sum |x||w|
 * (profiles/r11_wino_matrix.txt) the maximum error is 0.43-1.47x and the rms error 0.60-1.51x the direct fp32 kernel's: smaller on the long 3-D reductions (one
 * fused-multiply-add chain of K = 27 Cin there, 16 chains of 3 Cin here), larger on the 2-D forms and on short reductions, where the transforms' additions dominate. */
int forge_wino_weights(const float* wp, float* U, int Cout, int Cin, int kd, int transpose, forge_stream_t stream);
/* Weight gradient of the same convolution in the Winograd domain (training): dMm = A dy A^T (forge_wino_dy, the adjoint of the inverse
 * transform; dM [16][R][Cout]), dU[p][kd][co][ci] = sum_r dMm[p][r][co] (V1 | V2)[p][r + kd plane][ci] (forge_wino_wgrad: the weight-gradient
 * GEMM kernel of forge_conv_wgrad on 16 batched problems, dU [16][kd][Cout][C1+C2] ZERO-FILLED by the caller, fp32 atomics over voxel chunks),
 * dw[9 kd][Cout][Cin] += G^T dU G (forge_wino_dw: accumulates, like forge_conv_wgrad). V1 / V2 as in forge_wino_gemm (row strides = channel counts). */
int forge_wino_dy(const float* dy, int ldy, float* dM, int n, int D, int H, int W, int Cout, forge_stream_t stream);
int forge_wino_wgrad(const float* dMm, const float* V1, int C1, long long bs1, long long pt1, const float* V2, int C2, long long bs2,
                     long long pt2, float* dU, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
int forge_wino_dw(const float* dU, float* dw, int Cout, int Cin, int kd, forge_stream_t stream);
int forge_wino_input(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                     int nsum /* >1: transform the MEAN of nsum tensors sum_stride rows apart (models/encoder.py:62 view mean) */, long long sum_stride,
                     forge_stream_t stream);
/* An upstream gradient dy [n D H W][ld] (C channels) in BOTH transformed forms with one pass over it: V = B^T dy B (as forge_wino_input,
 * for the data-gradient point GEMMs) and dM = A dy A^T (as forge_wino_dy, for forge_wino_wgrad); both [16][n D H/2 W/2][C], dense.
 * (Backward of the reference's 3x3x3 convolutions under autograd: models/fusion.py:29-35, 61-68 via scripts/kubric_trainer.py:56.) */
int forge_wino_input_dy(const float* dy, int ld, float* V, float* dM, int n, int D, int H, int W, int C, forge_stream_t stream);
int forge_wino_gemm(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                    long long pt2, const float* U, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, int tile /* 0 = forge_wino_gemm_tile's rule */,
                    forge_stream_t stream);
/* The same pair with the inverse transform's ROW stage moved into the GEMM's epilogue (inference of models/fusion.py:29-35, 61-68 and models/encoder.py:36-40):
 * one workgroup runs the four points (i = 0..3, j) of a point column on its 64 x 128 tile and stores s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3 - the
 * operations forge_wino_output performs first, in its order - as Mm8 [2][4][R][Cout]: the point products cross HBM as 2x instead of 4x the output
 * tensor. forge_wino_output_half runs the column stage + the same fused tails on Mm8. Without a second addend the results are bitwise those of
 * forge_wino_gemm + forge_wino_output; a second addend (the shared input halves) arrives in the same 8-plane form and is added after the row stage. For the launches forge_wino_gemm_tile answers with 'B' (R >= 2048 tile rows, Cout > 64).
 * One output plane (R x Cout floats) must stay below 2 GiB (FORGE_ESHAPE otherwise): the planes are stored through 32-bit buffer offsets. */
int forge_wino_gemm_half(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                         long long pt2, const float* U, float* Mm8, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
int forge_wino_output_half(const float* Mm8, const float* Mm2_8 /* nullable second addend, 8 planes too */, long long bs2, long long pt2, const float* bias, const float* scale,
                           const float* shift, float slope, const float* residual, const float* aux_h, const float* aux_z, float* out, float* out2, float* out3,
                           int n, int D, int H, int W, int Cout, int ldo, int epilogue, forge_stream_t stream);
/* The depth nest: forge_wino_gemm's 16 point products Mm [16][R][Cout] of a THREE-depth-tap problem with a Winograd F(2, 3) over the depth taps
 * inside the GEMM kernel - four K loops of C1 + C2 per pair of planes (z, z + 1), z even, instead of six. Position k multiplies the operand
 * V[z-1] - V[z+1] | V[z] + V[z+1] | V[z+1] - V[z] | V[z] - V[z+2] (one fp32 addition of two planes of V, planes outside the grid are zero) with
 * Ud[p][k]; the pair's rows are (m0 + m1) + m2 and (m1 - m2) - m3. forge_wino_weights_dn makes Ud [16][4][Cout][Cin] = G_depth (x) (G w G^T) from the
 * packed weights wp [27][Cout][Cin], depth rows w0, (w0 + w1 + w2) / 2, (w0 - w1 + w2) / 2, w2, in float64 and rounded once. The result feeds
 * forge_wino_output like forge_wino_gemm's; it is rounded in another order and is not bitwise forge_wino_gemm's. Operands as forge_wino_gemm.
 * FORGE_EINVAL unless kd == 3, D is even, Ht Wt % 64 == 0 and C1, C2 are multiples of 32; one output plane must stay below 2 GiB (FORGE_ESHAPE). */
int forge_wino_gemm_dn(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                       long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
int forge_wino_weights_dn(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream);
/* The depth nest with F(4, 3): four K loops per plane pair become six per GROUP of four planes (1.5 per plane). Three entries:
 * forge_wino_input_dn4: forge_wino_input (same arguments: bs, nsum / sum_stride, ldv, ptv) plus the depth stage. V6 [16][n][D/4][6][H/2 W/2][C]; position k
 *   of group g combines the planes p_e = 4g - 1 + e, e = 0..5, of the batch element (zero outside ITS grid) per input element, in this order:
 *   q0 = 4 (p0 - p2) - (p2 - p4), q1 = (p3 + p4) - 4 (p1 + p2), q2 = (p4 - p3) + 4 (p1 - p2), q3 = (p4 - p2) + 2 (p3 - p1), q4 = (p4 - p2) - 2 (p3 - p1),
 *   q5 = 4 (p1 - p3) - (p3 - p5) (two rounded additions and one fused multiply-add with an exact product each), then B^T q B as forge_wino_input.
 * forge_wino_weights_dn4: Ud [16][6][Cout][Cin] = G_depth (x) (G w G^T) from wp [27][Cout][Cin], depth rows w0 / 4, -(w0 + w2 + w1) / 6, -(w0 + w2 - w1) / 6,
 *   (w0 / 4 + w2 + w1 / 2) / 6, (w0 / 4 + w2 - w1 / 2) / 6, w2; float64 throughout, rounded once.
 * forge_wino_gemm_dn4: the 16 point products Mm [16][R][Cout] of forge_wino_gemm from V6 operands (V1 | V2 along K; bs1 / bs2 / pt1 / pt2 in rows / floats of
 *   the V6 layout, 0 = dense) and Ud. Products m_k = V6[.][g][k] (x) Ud[p][k]; rows y0 = ((m1 + m2) + (m3 + m4)) + m0, y1 = (m1 - m2) + 2 (m3 - m4),
 *   y2 = (m1 + m2) + 4 (m3 + m4), y3 = ((m1 - m2) + 8 (m3 - m4)) + m5, where m0 and m5 are accumulated onto the bracket in front of them.
 *   FORGE_EINVAL, before any launch, unless kd == 3, D % 4 == 0, Ht Wt % 64 == 0, C1 and C2 are multiples of 32 and every operand and output plane
 *   stays within 32-bit buffer offsets. Feeds forge_wino_output; not bitwise forge_wino_gemm's result. */
int forge_wino_input_dn4(const float* in, int ld, long long bs, float* V6, int ldv, long long ptv, int n, int D, int H, int W, int C,
                         int nsum, long long sum_stride, forge_stream_t stream);
int forge_wino_weights_dn4(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream);
int forge_wino_gemm_dn4(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                        long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
/* The F(4, 3) depth nest with F(4, 3) along H as well ("dn4h"): tiles of 4 x 2 output voxels, Ht = H / 4, Wt = W / 2, 24 points p = 4 i + j (i = 0..5 the H point,
 * j = 0..3 the W point of F(2, 3)) - 3 multiplies per output against 4, operands and point products at 3/4 of forge_wino_gemm_dn4's bytes. Four entries:
 * forge_wino_input_dn4h: V [24][n][D/4][6][Ht Wt][C] (arguments as forge_wino_input_dn4). Per tile (th, tw) of group g the patch is the six rows 4 th - 1 .. 4 th + 4
 *   x the four columns 2 tw - 1 .. 2 tw + 2 of the six planes 4 g - 1 .. 4 g + 4 (zero outside the element's grid). Three stages, in this order:
 *   (1) depth, per patch element: forge_wino_input_dn4's six lines q0 .. q5 on the planes; (2) rows, per position k and patch column: THE SAME six lines on the
 *   six patch rows of q_k; (3) columns, per position and point row: w0 - w2, w1 + w2, w2 - w1, w1 - w3 (forge_wino_input's column stage). Every multiplier is
 *   a power of two: a float32 evaluation in this order reproduces the bits. FORGE_EINVAL unless D % 4 == 0, D >= 8, H % 4 == 0.
 * forge_wino_weights_dn4h: Ud [24][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G2(W) from wp [27][Cout][Cin]: forge_wino_weights_dn4's depth rows on every element,
 *   then the same six rows over the kernel's H taps, then w0, (w0 + w1 + w2) / 2, (w0 - w1 + w2) / 2, w2 over its W taps; float64 throughout, rounded once.
 * forge_wino_gemm_dn4h: forge_wino_gemm_dn4's launch with 24 batched problems on the grid (n, D, Ht, Wt): Mm [24][n D Ht Wt][Cout]. FORGE_EINVAL, before any
 *   launch, unless kd == 3, D % 4 == 0, D >= 8, Ht Wt % 64 == 0, C1 and C2 are multiples of 32 and every operand and output plane stays within 32-bit offsets.
 * forge_wino_output_dn4h: the inverse transform with the GRU tails of forge_wino_output (epilogue 2: gates, ldo == Cout / 2; 3: state; no second addend, no
 *   residual): over the six H points s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4, rows (s + S) + m0 | d + 2 D | s + 4 S | (d + 8 D) + m5 (the scalings
 *   fused, exact), then forge_wino_output's (s0 + s1) + s2 | (s1 - s2) - s3 over the four W points. FORGE_ESHAPE unless H % 4 == 0, W even, Cout % 8 == 0. */
int forge_wino_input_dn4h(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                          int nsum, long long sum_stride, forge_stream_t stream);
int forge_wino_weights_dn4h(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream);
int forge_wino_gemm_dn4h(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                         long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
int forge_wino_output_dn4h(const float* Mm, const float* bias, const float* scale, const float* shift, const float* aux_h, const float* aux_z, float* out,
                           float* out2, float* out3, int n, int D, int H, int W, int Cout, int ldo, int epilogue, forge_stream_t stream);
/* The F(4, 3) depth nest with F(4, 3) along H AND W ("dn4hw"): tiles of 4 x 4 output voxels, Ht = H / 4, Wt = W / 4, 36 points p = 6 i + j (i = 0..5 the H point,
 * j = 0..5 the W point) - 2.25 multiplies per output against dn4h's 3, operands and point products at 3/4 of its bytes. Four entries:
 * forge_wino_input_dn4hw: V [36][n][D/4][6][Ht Wt][C] (arguments as forge_wino_input_dn4h: bs, nsum / sum_stride, ldv, ptv). Per tile (th, tw) of group g the patch is
 *   the six planes 4 g - 1 .. 4 g + 4 x the six rows 4 th - 1 .. 4 th + 4 x the six columns 4 tw - 1 .. 4 tw + 4 (zero outside the element's grid, never the
 *   neighbouring element). Three stages, in this order, each forge_wino_input_dn4's six lines q0 .. q5: (1) depth, per patch element, on the planes; (2) rows, per
 *   position k and patch column, on the six patch rows of q_k; (3) columns, per position and point row i, on the six patch columns: V[6 i + j] = line j. Every
 *   multiplier is a power of two: a float32 evaluation in this order reproduces the bits. FORGE_EINVAL unless D % 4 == 0, D >= 8, H % 4 == 0, W % 4 == 0.
 * forge_wino_weights_dn4hw: Ud [36][6][Cout][Cin] = G4(depth) (x) G4(H) (x) G4(W) from wp [27][Cout][Cin]: forge_wino_weights_dn4's six depth rows on every element,
 *   then the same six rows over the kernel's H taps, then the same six rows over its W taps; float64 throughout, rounded once.
 * forge_wino_gemm_dn4hw: forge_wino_gemm_dn4h's launch with 36 batched problems on the grid (n, D, Ht, Wt): Mm [36][n D Ht Wt][Cout]; V1 | V2 along K, view strides as
 *   there. FORGE_EINVAL, before any launch, unless kd == 3, D % 4 == 0, D >= 8, Ht Wt % 64 == 0, C1 and C2 are multiples of 32 and every operand and output plane
 *   stays within 32-bit offsets.
 * forge_wino_output_dn4hw: the inverse transform with the GRU tails of forge_wino_output_dn4h (epilogue 2: gates, ldo == Cout / 2; 3: state; no second addend, no
 *   residual, as that entry). Over the six H points, per W point: s = m1 + m2, d = m1 - m2, S = m3 + m4, D = m3 - m4, rows (s + S) + m0 | d + 2 D | s + 4 S |
 *   (d + 8 D) + m5 (the scalings fused, exact); then THE SAME four lines over the six W points of each row; the tails run on the 4 x 4 voxels.
 *   FORGE_EINVAL unless H % 4 == 0 and W % 4 == 0; FORGE_ESHAPE unless Cout % 8 == 0. */
int forge_wino_input_dn4hw(const float* in, int ld, long long bs, float* V, int ldv, long long ptv, int n, int D, int H, int W, int C,
                           int nsum, long long sum_stride, forge_stream_t stream);
int forge_wino_weights_dn4hw(const float* wp, float* Ud, int Cout, int Cin, forge_stream_t stream);
int forge_wino_gemm_dn4hw(const float* V1, int C1, int ld1, long long bs1, long long pt1, const float* V2, int C2, int ld2, long long bs2,
                          long long pt2, const float* Ud, float* Mm, int n, int D, int Ht, int Wt, int Cout, int kd, forge_stream_t stream);
int forge_wino_output_dn4hw(const float* Mm, const float* bias, const float* scale, const float* shift, const float* aux_h, const float* aux_z, float* out,
                            float* out2, float* out3, int n, int D, int H, int W, int Cout, int ldo, int epilogue, forge_stream_t stream);
int forge_wino_gemm_tile(long long R, int Cout, int Cin);   /* the workgroup tile letter ('A'..'E', see forge_conv_igemm_plan) forge_wino_gemm uses for R tile rows per point, Cin = C1 + C2 */
int forge_wino_output(const float* Mm, const float* Mm2, long long bs2, long long pt2, const float* bias, const float* scale, const float* shift, float slope, const float* residual,
                      const float* aux_h, const float* aux_z, float* out, float* out2, float* out3, int n, int D, int H, int W, int Cout,
                      int ldo, int epilogue, forge_stream_t stream);

/* Weight gradient of forge_conv_igemm's convolution (training, scripts/kubric_trainer.py:56 -> torch conv backward):
 *   dw[t][co][ci] += sum_m dy[m][co] * x[voxel(m) + taps[t]][ci]      (x = channel concat of x1 | x2, zero outside the grid)
 * dy [M][ldy] is the upstream gradient of the conv output on the (n,D,H,W) row grid; x1/x2, is, Di.. as in forge_conv_igemm.
 * dw [ntaps][Cout][C1+C2] MUST be zero-filled: partial sums over voxel chunks are accumulated with fp32 atomics (the order of
 * the additions, hence the last bits, is not deterministic; forge_conv_wgrad_det below is). With two inputs C1 must be a multiple of 128.
 * The data gradient needs no extra entry point: it is forge_conv_igemm on dy with negated taps and wp[t][ci][co] (transposed).
 * Refusals: FORGE_EINVAL for null pointers, non-positive dims, ntaps outside 1..64, an x2 / C2 mismatch and any tap component outside
 * [-128, 127] (the kernels carry taps as signed bytes); FORGE_ESHAPE for channel counts or row strides that are no multiple of 4, ld < C,
 * two inputs with C1 % 128 != 0 and an operand spanning 2 GiB or more.
 */
int forge_conv_wgrad(const float* dy, int ldy, const float* x1, int C1, int ld1, long long bs1, const float* x2, int C2, int ld2,
                     long long bs2, float* dw, int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout,
                     const int* taps, int ntaps, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a5 / a7  direct convolution for TINY channel counts (Cin in {4, 8, 16}, Cout in 1..4): the last convolutions of the density head
 * (Conv3d(8, 1, 3), models/encoder.py:31) and of conv_rgb (Conv2d(8, 3, 5), models/volume_render.py:36). A matrix-core tile pads such
 * a layer to 16 or 32 channels on both sides (up to 128x the useful FLOPs); these are streaming problems and run on the vector ALUs.
 * Stride-1 "same" geometry on channels-last rows: in [M][ld_in], w [ntaps][Cout][Cin], taps (dz,dy,dx) inside the (n,D,H,W) grid, every
 * component in [-128, 127] (FORGE_EINVAL otherwise: the kernels carry taps as signed bytes).
 *   fwd    out[m][co] = act(bias[co] + sum_t sum_ci w[t][co][ci] in[m + tap_t][ci])     (bias nullable; act = LeakyReLU(slope):
 *          slope 1 = none, 0 = ReLU - the inference path fuses the layer's trailing ReLU)
 *   dgrad  dx[m][ci]  = sum_t sum_co w[t][co][ci] dy[m - tap_t][co]
 *   wgrad  dw[t][co][ci] += sum_m dy[m][co] x[m + tap_t][ci]                              (dw zero-filled by the caller; fp32 atomics)
 */
int forge_conv_direct_fwd(const float* in, int ld_in, const float* w, const float* bias, float slope, float* out, int ld_out,
                          int n, int D, int H, int W, int Cin, int Cout, const int* taps, int ntaps, forge_stream_t stream);
int forge_conv_direct_dgrad(const float* dy, int ld_dy, const float* w, float* dx, int ld_dx,
                            int n, int D, int H, int W, int Cin, int Cout, const int* taps, int ntaps, forge_stream_t stream);
int forge_conv_direct_wgrad(const float* dy, int ld_dy, const float* x, int ld_x, float* dw,
                            int n, int D, int H, int W, int Cin, int Cout, const int* taps, int ntaps, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deterministic mode: bitwise-reproducible counterparts of the entry points whose partial sums are added with fp32 atomics
 * (forge_conv_wgrad, forge_wino_wgrad, forge_conv_direct_wgrad, the dxf output of forge_rotate_bwd / forge_rotate_bwd_slots).
 * Each _det function takes its counterpart's arguments plus (accumulate, ws, ws_bytes) in front of the stream:
 *   accumulate = 0   the output (dw / dU / dxf) is WRITTEN, every element: no zero-fill needed, prior contents (NaN included) are ignored
 *   accumulate = 1   out = prior + S with exactly one fp32 add per element, S being what accumulate = 0 writes
 *   ws, ws_bytes     caller-owned scratch, 16-byte aligned, of at least the matching *_det_ws_bytes(...) bytes (checked: FORGE_EINVAL)
 * The kernels store per-chunk partial sums into slabs of ws (plain stores, zeros included) and a second launch on the same stream sums
 * the slabs in chunk order (float64, rounded once). The split - and with it the order of every addition - depends on the shape arguments
 * only: not on ws_bytes, timing or the device's state; the same inputs give the same bits in any process on any MI355X. One launch's
 * slab set is capped at 64 MiB by lowering the chunk count. Outputs must be 16-byte aligned (dw, dU: any torch allocation; dxf [n][12]).
 * The *_det_ws_bytes queries are host-only (no device, no stream) and return < 0 for arguments the launch would reject; the query of
 * forge_conv_wgrad_det takes the host tap table because the kernel choice depends on the tap geometry. dvox of forge_rotate_bwd_det is the
 * same deterministic gather as forge_rotate_bwd's; with dxf NULL no workspace is used.
 */
int forge_conv_wgrad_det(const float* dy, int ldy, const float* x1, int C1, int ld1, long long bs1, const float* x2, int C2, int ld2,
                         long long bs2, float* dw, int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout,
                         const int* taps, int ntaps, int accumulate, void* ws, long long ws_bytes, forge_stream_t stream);
long long forge_conv_wgrad_det_ws_bytes(int C1, int C2, int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout,
                                        const int* taps, int ntaps);
/* Host-only, like the query above: what forge_conv_wgrad (det = 0) or forge_conv_wgrad_det (det = 1) launches for dense operands of this
 * shape - the dispatch itself with the launch switched off, refusals included (< 0). plan[8]:
 *   [0] kernel family  1 conv_wgrad_kernel<CIW, TG>  2 conv_wgrad_small_kernel  3 conv_wgrad_lines_kernel on the 32x32x2 MFMA  4 on the 16x16x4 MFMA <CIT, IS, .., NWV>
 *   [1] CIW (128 / 64 / 32) or CIT (16 / 32); 32 for families 2, 3      [2] TG (1 / 2 / 4) or IS (1 / 2); taps per wave (4) for family 2
 *   [3] waves per workgroup (NWV)                                       [4] workgroups of the launch
 *   [5] voxel chunks (families 1, 2) or persistent workgroups walking the 32-voxel segments (3, 4): the slab count of the deterministic mode
 *   [6] mchunk, voxels per chunk (0 for families 3, 4)                  [7] (dz, dy) lines (families 3, 4) */
int forge_conv_wgrad_plan(int C1, int C2, int n, int D, int H, int W, int is, int Di, int Hi, int Wi, int Cout, const int* taps, int ntaps,
                          int det, long long* plan);
int forge_wino_wgrad_det(const float* dMm, const float* V1, int C1, long long bs1, long long pt1, const float* V2, int C2, long long bs2,
                         long long pt2, float* dU, int n, int D, int Ht, int Wt, int Cout, int kd, int accumulate, void* ws, long long ws_bytes,
                         forge_stream_t stream);
long long forge_wino_wgrad_det_ws_bytes(int C1, int C2, int n, int D, int Ht, int Wt, int Cout, int kd);
int forge_conv_direct_wgrad_det(const float* dy, int ld_dy, const float* x, int ld_x, float* dw, int n, int D, int H, int W, int Cin, int Cout,
                                const int* taps, int ntaps, int accumulate, void* ws, long long ws_bytes, forge_stream_t stream);
long long forge_conv_direct_wgrad_det_ws_bytes(int n, int D, int H, int W, int Cin, int Cout, int ntaps);
int forge_rotate_bwd_det(const float* dout, const float* vox, const float* xf, const int* mode, float* dvox, float* dxf,
                         int n, int C, int D, int H, int W, int accumulate, void* ws, long long ws_bytes, forge_stream_t stream);
long long forge_rotate_bwd_det_ws_bytes(int n, int C, int D, int H, int W);
int forge_rotate_bwd_slots_det(const float* dout, const float* vox, const float* xf, const int* mode, const int* src_slot,
                               float* dvox, float* dxf, int n, int C, int D, int H, int W, int accumulate, void* ws, long long ws_bytes,
                               forge_stream_t stream);
long long forge_rotate_bwd_slots_det_ws_bytes(int n, int C, int D, int H, int W);

/* ---------------------------------------------------------------------------------------------
 * a4 (training)  element-wise halves of the ConvGRU cell, models/fusion.py:29-35 under autograd. Inference fuses them into
 * forge_conv_igemm's GRU epilogues; with an autograd graph the two convolutions run with the bias epilogue and each half of the
 * cell is one kernel per direction. All arrays are channels-last rows [M][C] fp32, C % 4 == 0, g / dg are [M][2C] (update | reset).
 *   gates fwd: z = sigmoid(g[:, :C]), r = sigmoid(g[:, C:]), hr = h * r
 *   state fwd: cand = tanh(c) (written over c), hn = h (1 - z) + cand z
 *   state bwd: dh = dhn (1 - z), dz = dhn (cand - h), dc = dhn z (1 - cand^2)        (dhn rows may be strided: ld_dhn floats)
 *   gates bwd: dg = (dz z (1 - z) | dhr h r (1 - r)), dh_out = dh + dhr r  (dhr rows may be strided: ld_dhr floats; dh_out NULL = in
 *              place over dh, else rows of stride ld_dh_out - it may alias dhr, which lets the sum land beside the x-gradient half)
 */
int forge_gru_gates_fwd(const float* g, const float* h, float* z, float* r, float* hr, long long M, int C, forge_stream_t stream);
int forge_gru_state_fwd(float* c_cand, const float* h, const float* z, float* hn, long long M, int C, forge_stream_t stream);
/* dc_acc / dg_acc (acc_mode 0: unused, 1: written, 2: added to): a second copy of dc / dg for the gradient of a convolution INPUT HALF that several
 * fusions share (model_single_pose_estimator.py:108-120 fuses views (0,1,2), (3,4), (0..4) of the same features): rows of batch element n land at
 * acc + (n acc_bs + row within the volume of `vol` rows) x (C | 2C) floats, i.e. view ti of a [b][t] stack is acc = base + ti vol ld, acc_bs = t vol. */
int forge_gru_state_bwd(const float* dhn, int ld_dhn, const float* h, const float* z, const float* cand, float* dh, float* dz, float* dc,
                        long long M, int C, float* dc_acc, long long acc_bs, long long vol, int acc_mode, forge_stream_t stream);
int forge_gru_gates_bwd(const float* dz, const float* dhr, int ld_dhr, const float* h, const float* z, const float* r,
                        float* dg, float* dh, float* dh_out, int ld_dh_out, long long M, int C, float* dg_acc, long long acc_bs, long long vol,
                        int acc_mode, forge_stream_t stream);

/* Train-mode BatchNorm (+ LeakyReLU / ReLU) on channels-last rows (training path; torch.nn.BatchNorm{2,3}d(train) + activation of
 * models/fusion.py:49-58, models/encoder.py:16-40, models/volume_render.py:29-37 and the torchvision bottlenecks):
 *   fwd   batch statistics over the M rows (float64 sums), y = lrelu((x - mean) invstd gamma + beta, slope); mean / invstd [C] are stored for the
 *         backward; running_mean / running_var (nullable) are updated in place with `momentum` (unbiased variance), as nn.BatchNorm does
 *   bwd   g = dy * (pre-activation > 0 ? 1 : slope); dx = gamma invstd (g - mean(g) - xhat mean(g xhat)); dgamma = sum g xhat, dbeta = sum g
 * x / y / dy / dx rows [M][ld] fp32, C % 4 == 0; gamma / beta nullable (1 / 0); slope 1 = no activation, 0 = ReLU; ws = forge_bn_ws_doubles(C)
 * doubles of scratch (one float64 partial per reduction block, summed by a second kernel in a fixed order: deterministic, no atomics).
 * Residual form (torchvision Bottleneck tail, out = relu(bn3(conv3) + identity)): res [M][ldres] (nullable) is added before the activation
 * in the same pass; the backward then takes the forward's OUTPUT y (mask = y > 0, valid for slope >= 0) and also writes d res = g to dres
 * (nullable). num_batches_tracked (nullable, int64 on the device) is incremented by the forward's finalize step - no separate launch. */
int forge_bn_ws_doubles(int C);
/* Column sums out[c] = sum_m x[m][c] of a row-major [M][C] matrix with row stride ldx (floats): the bias gradient of a convolution (torch:
 * dy.sum over every dimension but the channels). float64 partial sums in a fixed order (deterministic); ws = forge_bn_ws_doubles(C) doubles. */
int forge_colsum(const float* x, int ldx, float* out, double* ws, long long M, int C, forge_stream_t stream);
int forge_bn_train_fwd(const float* x, int ldx, const float* gamma, const float* beta, float eps, float slope, float* y, int ldy,
                       float* mean, float* invstd, float* running_mean, float* running_var, float momentum, double* ws,
                       long long M, int C, const float* res, int ldres, long long* num_batches_tracked,
                       int nblk_pre /* > 0: ws already holds that many partial rows [2][C] - forge_conv_igemm's `stats` by-product - and the statistics pass is skipped */,
                       forge_stream_t stream);
int forge_bn_train_bwd(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                       const float* invstd, float slope, float* dx, int lddx, float* dgamma, float* dbeta, double* ws, long long M, int C,
                       const float* y, int ldy, float* dres, int lddres, forge_stream_t stream);
/* SyncBatchNorm (torch.nn.SyncBatchNorm.convert_sync_batchnorm, kubric_train_pose_3D.py:119, kubric_train_joint.py:136): the same kernels
 * with ONE all-reduce (SUM) of 2 C doubles (+ the row count) between the reduction and the apply step, issued by the caller (RCCL):
 *   forge_bn_sync_stats       ws[0 .. 2C) = this rank's (sum x, sum x^2) over its M rows          -> all-reduce -> totals, M_total
 *   forge_bn_sync_fwd_apply   mean / invstd (written) and running statistics (updated, unbiased over M_total) from the totals; y as above
 *   forge_bn_sync_bwd_reduce  ws[0 .. 2C) = this rank's (sum g, sum g xhat); dgamma / dbeta = those LOCAL sums (torch's SyncBatchNorm
 *                             does the same: DDP averages parameter gradients afterwards)           -> all-reduce -> totals
 *   forge_bn_sync_bwd_apply   dx = gamma invstd (g - totals_g / M_total - xhat totals_gx / M_total)
 * ws as for forge_bn_train_fwd (forge_bn_ws_doubles(C) doubles); totals may alias ws. M_total = 0: the all-rank row count is read from
 * device memory at totals[2 C] (a double, all-reduced with the sums: no host round trip per layer). With M_total = M and no all-reduce the four calls
 * reproduce forge_bn_train_fwd / _bwd bit for bit. */
int forge_bn_sync_stats(const float* x, int ldx, double* ws, long long M, int C, int nblk_pre /* as forge_bn_train_fwd */, forge_stream_t stream);
int forge_bn_sync_fwd_apply(const float* x, int ldx, const float* gamma, const float* beta, float eps, float slope, float* y, int ldy,
                            float* mean, float* invstd, float* running_mean, float* running_var, float momentum, const double* totals,
                            long long M_total, long long M, int C, const float* res, int ldres, long long* num_batches_tracked, forge_stream_t stream);
/* Eval-mode BatchNorm (+ residual) + LeakyReLU(slope) on channels-last rows UNDER AUTOGRAD with trainable gamma / beta (a fine-tune that keeps
 * BatchNorm layers in eval mode: torch's F.batch_norm(training=False), which the reference reaches through nn.BatchNorm*.forward):
 * mean = running_mean, invstd = 1 / sqrt(running_var + eps) are written for the backward, the running statistics are only read.
 * Backward = forge_bn_sync_bwd_reduce (dgamma, dbeta) + forge_bn_sync_bwd_apply with all-zero totals (dx = gamma invstd g: the statistics
 * do not depend on x). */
int forge_bn_eval_fwd(const float* x, int ldx, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, float slope, float* y, int ldy, float* mean, float* invstd, long long M, int C, const float* res, int ldres,
                      forge_stream_t stream);
int forge_bn_sync_bwd_reduce(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                             const float* invstd, float slope, float* dgamma, float* dbeta, double* ws, long long M, int C,
                             const float* y, int ldy, forge_stream_t stream);
int forge_bn_sync_bwd_apply(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                            const float* invstd, float slope, float* dx, int lddx, const double* totals, long long M_total, long long M, int C,
                            const float* y, int ldy, float* dres, int lddres, forge_stream_t stream);

/* Backward of forge_conv_igemm's epilogue 1 (folded eval-BatchNorm + LeakyReLU / ReLU) for frozen-weight optimisation loops (pose
 * refinement, kubric_eval.py:412-530): dx[m][c] = dy[m][c] * scale[c] * (y[m][c] > 0 ? 1 : slope), y = the forward OUTPUT (its sign
 * is the pre-activation's for slope >= 0). Rows may be strided (ld_* floats); scale nullable (= 1). The data gradient of the
 * convolution itself is forge_conv_igemm on dx with negated taps and transposed weights. */
int forge_affine_act_bwd(const float* dy, int ld_dy, const float* y, int ld_y, const float* scale, float slope, float* dx, int ld_dx,
                         long long M, int C, forge_stream_t stream);

/* Single-head dot-product attention out = softmax(q k^T) v, fp32 on the matrix cores with the N x N matrix kept in registers (online softmax over
 * 32-key tiles). Replaces `Attention.forward` / `Attention.get_attn` + the matmul behind it (models/model_utils.py:207-229, called by
 * models/pose_estimator_3d.py:116-144 with N = 4096 tokens per volume pair) in predicted-pose INFERENCE; torch computes the same sums with the matrix
 * materialised three times. Unscaled logits, as the reference. q [B][Nq][d], k [B][Nk][d], v [.][Nk][d] with a batch stride of v_batch_rows rows
 * (0 = one v shared by all batch elements: the positional table of the cross attention), out [B][Nq][d]; d = 64, Nq and Nk multiples of 64. */
int forge_attention_fwd(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, int B, int Nq, int Nk, int d,
                        forge_stream_t stream);

/* The differentiable pair of forge_attention_fwd, for TRAINING the pose estimator (opt-in on the Python side: ops.set_attention_training).
 * forge_attention_fwd_lse: forge_attention_fwd (same kernel, same launch rule, `out` bit for bit the same) that also writes
 *   lse[B][Nq] = ln sum_keys exp(q . k), the natural-log sum-exp of the unscaled logits - all the backward needs to recompute the softmax.
 * forge_attention_bwd: gradients of out = softmax(q k^T) v for the upstream gradient dout [B][Nq][d]. The softmax P = exp(q k^T - lse) is
 *   recomputed tile by tile from the saved lse; nothing of size Nq x Nk is stored. Three launches on `stream`, no atomics - the results are
 *   bitwise reproducible from run to run:
 *     delta_ws[B][Nq] = sum_c dout out          (workspace of B Nq floats owned by the caller; nothing is allocated inside)
 *     dq = dS k            with dS = P o (dout v^T - delta)          (one wave per 32 queries walks the key tiles)
 *     dk = dS^T q,  dv = P^T dout                                    (one wave per 32 keys walks the query tiles)
 *   The dq pass also sums each row of dS (0 in exact arithmetic; with delta taken from the fp32 `out` it is the forward's rounding) and of P,
 *   accumulates P k, and removes the residual: rho = sum dS / sum P, dq -= rho (P k), delta_ws += rho for the second pass - so that every row of
 *   dS sums to zero as in a softmax backward that keeps the matrix. 8 contractions of 2 B Nq Nk d FLOPs with dv, 7 without.
 *   dq [B][Nq][d], dk [B][Nk][d] and dv [B][Nk][d] (dense) are written in full: no pre-zeroing, no accumulation into them.
 *   dv may be NULL: the dv chain is skipped. With one v shared by the batch (v_batch_rows = 0: the positional table, a constant) dv MUST be
 *   NULL (FORGE_EINVAL otherwise).
 * Domain and layouts as forge_attention_fwd: d = 64, Nq and Nk multiples of 64. */
int forge_attention_fwd_lse(const float* q, const float* k, const float* v, long long v_batch_rows, float* out, float* lse, int B, int Nq, int Nk,
                            int d, forge_stream_t stream);
int forge_attention_bwd(const float* q, const float* k, const float* v, long long v_batch_rows, const float* out, const float* lse,
                        const float* dout, float* dq, float* dk, float* dv, float* delta_ws, int B, int Nq, int Nk, int d, forge_stream_t stream);

/* Multi-head attention out = softmax(scale q k^T) v per head, for the six attention blocks of the 2-D pose estimator
 * (`MultiHeadAttention`, models/model_utils.py:258-342: 4 heads of 64 channels, scale = 64^-1/2; opt-in on the Python side:
 * ops.set_multihead_attention). The kernels of the three entry points above with two additions - those entry points are their H = 1, row stride
 * 64, scale = 1 case, bit for bit:
 *   head addressing: the projections stay as the Linear layers wrote them, [B][N][H*64] rows. Batch index b*H + h reads row r of q at
 *     q + b*q_bs + r*q_rs + 64*h, and k (k_bs, k_rs), v (v_bs, v_rs) and out (out_bs, out_rs) alike: no head-split copy, no head-merge copy.
 *     Strides are in floats, the channel stride is 1; slices of a wider tensor (one fused [B][N][3*H*64] projection) are addressed as they are.
 *     Every stride must be a non-negative multiple of 4 (FORGE_ESHAPE) and q, k, v, out 16-byte aligned (FORGE_EINVAL): float4 access. Rows of
 *     out must not overlap (out_rs >= H*64, out_bs >= Nq*out_rs for B > 1).
 *   scale: a finite positive logit scale (FORGE_EINVAL otherwise), folded into the multiply q gets anyway (q * scale * log2 e); in the backward
 *     dq and dk carry it, applied after the row-residual correction of the dq pass (dq = scale * (dS k - rho P k)).
 * Dense buffers: lse [B][H][Nq] and delta_ws [B][H][Nq] (workspace of the caller), dout [B][Nq][H*64], dq [B][Nq][H*64], dk and dv [B][Nk][H*64].
 * forge_attention_mh_fwd: lse may be NULL (inference: not stored; `out` has the same bits either way).
 * forge_attention_mh_bwd: dv may be NULL (not wanted: the dv chain is skipped). Three launches, no atomics, bitwise reproducible; dq, dk, dv are
 *   written in full. FLOPs: 4 B H Nq Nk d forward, 16 (14 without dv) B H Nq Nk d backward.
 * The two-/four-part launch rule of the single-head entry points applies to B*H batch indices. d = 64, H >= 1, Nq and Nk multiples of 64
 * (FORGE_ESHAPE); null pointers other than the two named are FORGE_EINVAL. */
int forge_attention_mh_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int B, int H, int Nq, int Nk, int d,
                           long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs, long long v_rs, long long out_bs,
                           long long out_rs, float scale, forge_stream_t stream);
int forge_attention_mh_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq,
                           float* dk, float* dv, float* delta_ws, int B, int H, int Nq, int Nk, int d, long long q_bs, long long q_rs,
                           long long k_bs, long long k_rs, long long v_bs, long long v_rs, long long out_bs, long long out_rs, float scale,
                           forge_stream_t stream);

/* Token-row layers of the pose estimators' transformer blocks (csrc/token.hip; opt-in on the Python side: ops.set_token_layers): LayerNorm,
 * Linear and exact-erf GELU on fp32 rows, the GEMMs on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain).
 * Common rules: fp32; channel stride 1; row strides (ld*, in floats) multiples of 4 and at least the row's width (FORGE_ESHAPE); every pointer
 * 16-byte aligned (FORGE_EINVAL); R >= 1 rows of any count (the last 32-row tile is masked; R < 1 is FORGE_EINVAL); K and N multiples of 64, at
 * most 1024, and K <= 256 wherever a LayerNorm is involved - its normalised 32-row tile lives in LDS (FORGE_ESHAPE). w [N][K] is nn.Linear's
 * layout, dense. Every check runs before the first launch; nothing is allocated and nothing synchronises (capturable into a hipGraph). No
 * atomics: every result is bitwise reproducible.
 *
 * forge_token_linear_fwd: y[R][N] = act( LN?(x[R][K]) w^T + bias ) (+ residual), one launch.
 *   LayerNorm prologue iff gamma != NULL (beta then required, eps finite and >= 0): torch's definition - mean and biased variance per row,
 *     (x - mean) rstd gamma + beta with rstd = 1 / sqrt(var + eps) - the statistics in two passes over the resident row (mean, then the centred
 *     squares). stats [R][2] nullable (only with the prologue): (mean, rstd) per row, for the backward.
 *   act: FORGE_TOKEN_ACT_NONE or FORGE_TOKEN_ACT_GELU (0.5 v (1 + erf(v / sqrt 2)), nn.GELU()'s default); anything else FORGE_EINVAL.
 *     pre [R][N] dense, nullable: the pre-activation (after the bias), for the backward.
 *   bias [N] and residual (row stride ldr) nullable. y (row stride ldy) may be a slice of a wider tensor (a q|k|v slab): the bits do not depend
 *     on the strides. LN-prologue + linear gives the bits of forge_layer_norm_fwd followed by the plain linear. FLOPs 2 R K N.
 * forge_layer_norm_fwd: y[R][K] = LN(x), the prologue's device code stand-alone; stats nullable.
 * forge_token_linear_bwd: for the upstream dy [R][N] (row stride lddy) and g = dy o act'(pre), GELU'(v) = Phi(v) + v phi(v):
 *     dbias [N] = sum_r g      dw [N][K] = sum_r g[r][n] xn[r][k]   (xn recomputed from x and stats: never stored)      dxn = g w
 *     through the LayerNorm (gamma, beta, stats all given, or all NULL), xh = (x - mean) rstd:
 *     dgamma [K] = sum_r dxn o xh    dbeta [K] = sum_r dxn    dx = rstd (dxn o gamma - mean_k(dxn o gamma) - xh mean_k(dxn o gamma o xh))
 *   dx [R][K] dense, dw, dbias, dgamma, dbeta are each nullable: that chain is skipped (dbias needs dw: it is a by-product of the dW pass,
 *   FORGE_EINVAL otherwise; dgamma / dbeta without a LayerNorm are FORGE_EINVAL). pre is required with GELU. The residual's gradient is dy itself.
 *   The sums over rows split the rows into chunks by a plan that depends on (R, K, N) alone (forge_token_rows_plan: `chunks` chunks of
 *   `chunk_rows` rows for dw / dbias; about 256 chunks for dgamma / dbeta); partial tiles go to the caller's workspace and are added in chunk
 *   order. ws: forge_token_linear_bwd_ws_bytes(R, K, N, ln) bytes (ln = 1 with the LayerNorm prologue; may be 0, ws is then not read; -1 outside
 *   the domain); a smaller ws_bytes is FORGE_EINVAL. Up to 6 launches. FLOPs 2 R K N for dxn and for dw each.
 * forge_layer_norm_bwd: dx [R][K] dense, dgamma, dbeta (each nullable) of forge_layer_norm_fwd for dy (row stride lddy);
 *   ws: forge_layer_norm_bwd_ws_bytes(R, K) bytes, needed for dgamma / dbeta. */
#define FORGE_TOKEN_ACT_NONE 0
#define FORGE_TOKEN_ACT_GELU 1
int forge_token_linear_fwd(const float* x, long long ldx, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                           const float* residual, long long ldr, float* y, long long ldy, float* pre, float* stats, int R, int K, int N, int act,
                           forge_stream_t stream);
int forge_layer_norm_fwd(const float* x, long long ldx, const float* gamma, const float* beta, float eps, float* y, long long ldy, float* stats,
                         int R, int K, forge_stream_t stream);
int forge_token_rows_plan(int R, int K, int N, int* chunks, int* chunk_rows);
long long forge_token_linear_bwd_ws_bytes(int R, int K, int N, int ln);
int forge_token_linear_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* w, const float* gamma, const float* beta,
                           const float* stats, const float* pre, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta, float* ws,
                           long long ws_bytes, int R, int K, int N, int act, forge_stream_t stream);
long long forge_layer_norm_bwd_ws_bytes(int R, int K);
int forge_layer_norm_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* gamma, const float* stats, float* dx,
                         float* dgamma, float* dbeta, float* ws, long long ws_bytes, int R, int K, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a1  ResNet stem helpers (torchvision conv1/bn1/relu/maxpool behind models/encoder.py:71-73).
 * forge_im2col_nchw: img [N][C][H][W] -> patch rows out [N*Ho*Wo][Kpad], k = (ky*kw + kx)*C + c, zeros outside the image and
 *   for k >= kh*kw*C; Ho = (H + 2 pad - kh)/stride + 1. The 7x7/s2 stem conv then runs as forge_conv_igemm with one tap and
 *   C1 = Kpad (BN + ReLU in its epilogue).
 * forge_maxpool2d_nhwc: in [N][H][W][C] -> out [N][Ho][Wo][C], window k, -inf padding (nn.MaxPool2d semantics), C % 4 == 0.
 *   A NaN inside a window is that window's result, as in nn.MaxPool2d.
 */
int forge_im2col_nchw(const float* img, float* out, int N, int C, int H, int W, int kh, int kw, int stride, int pad,
                      int Kpad, forge_stream_t stream);
int forge_maxpool2d_nhwc(const float* in, float* out, int N, int H, int W, int C, int k, int stride, int pad,
                         forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f1  squared-error sums of the reconstruction losses (scripts/kubric_compute_loss.py:26-29, 136-139: four F.mse_loss terms on
 * reshaped / repeated tensors) in one pass over the rendered maps, and their backward.
 *   pred    [B][Vp][C][H][W] addressed with element strides (sn per view, sc, sh, sw): the rgb maps are channels-last memory behind
 *           an NCHW view (conv_rgb's output), the masks plain NCHW
 *   target  [B][Vt][C][H][W] contiguous; rendered view v of scene b is compared with target view v % Vt and counted in group
 *           v / gsize (GT-pose model: Vp = 2t, Vt = gsize = t; joint model: Vp = Vt = 2t, gsize = t); at most 4 groups
 *   fwd     partial [forge_sse_groups_blocks()][G]: per-workgroup sums of (pred - target)^2 (fixed reduction tree; the caller adds
 *           the rows in a fixed order: deterministic, no atomics)
 *   bwd     dpred (same layout as pred) = coef[group] * (pred - target)
 */
int forge_sse_groups_blocks(void);
int forge_sse_groups_fwd(const float* pred, long long sn, long long sc, long long sh, long long sw, const float* target,
                         float* partial, int B, int Vp, int Vt, int gsize, int C, int H, int W, forge_stream_t stream);
int forge_sse_groups_bwd(const float* pred, long long sn, long long sc, long long sh, long long sw, const float* target,
                         const float* coef, float* dpred, int B, int Vp, int Vt, int gsize, int C, int H, int W, forge_stream_t stream);

/* f2  torch.optim.Adam (betas, eps; no weight decay / amsgrad) on one SMALL tensor in one launch, the step count `step` [1] (float) kept and
 * advanced on the device: the pose-refinement loop (kubric_eval.py:440-449) optimises b (t-1) x 7 numbers, for which the capturable torch
 * optimiser issues ~30 launches inside the captured iteration. param / exp_avg / exp_avg_sq [n] updated in place. */
int forge_adam_small(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* step, int n, float lr, float beta1, float beta2,
                     float eps, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3  VGG-16 perceptual loss (models/perceptual_loss.py:23-44: repeat to 3 channels, (x - mean) / std, bilinear resize to 224^2,
 * VGG-16 features[:23] with an L1 term at relu1_2 / relu2_2 / relu3_3 / relu4_3). The ten 3x3 convolutions run on forge_conv_igemm /
 * forge_wino_*, the max-pools on forge_maxpool2d_nhwc, the ReLU masks inside a block on forge_affine_act_bwd; these entries are the rest.
 *   prep_fwd  rows [(b ? 2N : N) Ho Wo][32] = conv1_1's patch rows (forge_im2col_nchw's k-order, k = (ky*3 + kx)*3 + c, 3x3 pad 1,
 *             zero for k >= 27) of the prepared images: images a[0..N) then b[0..N), each [N][C][Hi][Wi] read through element strides
 *             (C = 1 is repeated to 3), normalised by the DEVICE scalars mean[3] / std[3], resized with ATen's bilinear arithmetic
 *             (align_corners = False) when resize = 1 (else Ho = Hi, Wo = Wi). b nullable.
 *   prep_bwd  the adjoint: din [N][C][Hi][Wi] (element strides sn..sw) from g, the gradient of the prepared image as channels-last rows
 *             [N][Ho][Wo][ldg] (channel c at column c); a deterministic gather per source pixel, divided by std, summed over the three
 *             repeated channels when C = 1.
 *   l1        partial [forge_l1_partial_blocks()] = per-workgroup sums of |x - y| over n floats (x, y 16-byte aligned); fixed reduction
 *             tree, the caller adds the rows in a fixed order.
 *   tap_bwd   d_pre = (maxpool2x2_bwd(g_next) + coef[0] sign(x - y)) * (x > 0) on channels-last rows [N][H][W][C], x = the tap's
 *             post-ReLU output. The pool backward recomputes each window's winner from x (ATen: first maximum in row-major order, NaN
 *             wins); g_next [N][H/2][W/2][C] nullable (no following block), coef nullable (no L1 term at this tap; y is then unused).
 */
int forge_vgg_prep_fwd(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn,
                       long long b_sc, long long b_sh, long long b_sw, const float* mean, const float* std, float* rows, int N, int C,
                       int Hi, int Wi, int Ho, int Wo, int resize, forge_stream_t stream);
int forge_vgg_prep_bwd(const float* g, int ldg, const float* std, float* din, long long sn, long long sc, long long sh, long long sw,
                       int N, int C, int Hi, int Wi, int Ho, int Wo, int resize, forge_stream_t stream);
int forge_l1_partial_blocks(void);
int forge_l1_partial(const float* x, const float* y, long long n, float* partial, forge_stream_t stream);
int forge_vgg_tap_bwd(const float* x, const float* y, const float* g_next, const float* coef, float* d_pre, int N, int H, int W, int C,
                      forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f4  Image metrics of the evaluation protocol (utils/eval_utils.py:compute_img_metric, kubric_eval.py's lpips.LPIPS(net="vgg")). Images
 * a, b are [N][C][H][W] float32 read through element strides; image n of a is scored against image n of b. Each entry writes per-workgroup
 * partial sums into the caller's slab and sums them in a fixed order in a second launch: no atomics, bitwise reproducible, no allocation.
 *   psnr          out[n] (float64) = 10 log10(data_range^2 / mse), mse over C H W elements in float64; mse = 0 gives +inf.
 *                 partial: N * forge_metric_blocks() doubles.
 *   ssim          out[n] (float64) = mean over channels and over all valid 7x7 windows of skimage's SSIM map (uniform window, sample
 *                 covariance 49/48, K1 = 0.01, K2 = 0.03); H, W >= 7. partial: N * C * forge_ssim_tiles(H, W) doubles.
 *   ssim_tiles    partials per (image, channel) of forge_ssim, -1 when H or W < 7.
 *   lpips_tap     one LPIPS tap: f [2N][HW][C] channels-last (image n against image n + N), C in {64, 128, 256, 512}, w [C] the lin weights,
 *                 f and w 16-byte aligned; partial [N][forge_metric_blocks()] = partial sums over pixels of
 *                 sum_c w[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2.
 *   lpips_final   out[n] (float32) = sum over the 5 taps k of (sum of partial[k][n][*]) / hw_k; partial [5][N][forge_metric_blocks()].
 */
int forge_metric_blocks(void);
int forge_ssim_tiles(int H, int W);
int forge_psnr(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn, long long b_sc,
               long long b_sh, long long b_sw, int N, int C, int H, int W, double data_range, double* partial, double* out, forge_stream_t stream);
int forge_ssim(const float* a, long long a_sn, long long a_sc, long long a_sh, long long a_sw, const float* b, long long b_sn, long long b_sc,
               long long b_sh, long long b_sw, int N, int C, int H, int W, double data_range, double* partial, double* out, forge_stream_t stream);
int forge_lpips_tap(const float* f, int N, int HW, int C, const float* w, double* partial, forge_stream_t stream);
int forge_lpips_finalize(const double* partial, int N, int hw0, int hw1, int hw2, int hw3, int hw4, float* out, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f5  Camera synchronisation of the evaluation protocol (kubric_eval.py:95-145 `sync_pose`): utils/sync_utils.py:76-191
 * camera_synchronization(Ps, confidence, N, squares, so3_projection=True, normalize_confidences=True, double=True, center_first_camera=...).
 *   P      [B][E][4][4] pairwise extrinsics i -> j of edge e = (pairs[e][0], pairs[e][1]), row-major float32
 *   conf   [B][E] confidences
 *   pairs  [E][2] DEVICE int32 (i, j): i != j, both < N, no pair twice in either order, every view in some pair (the caller's duty; an
 *          entry outside 0..N-1 is skipped, never followed)
 *   center the view whose block column of L^(2^squares) is kept: 0 for center_first_camera=True, N / 2 otherwise
 *   out    [B][N][4][4] float32: the synchronised extrinsics, rotation blocks projected onto SO(3)
 *   sv     [B][N][3] float64, nullable: singular values (descending) of the rotation blocks BEFORE the projection
 *   status [B] int32 bit set: 1 a mass entry <= 0 (or NaN) - the reference's assertion "2**squares, or the set of edges, is too small";
 *          2 for some view sigma_min / sigma_max < rank_tol or sigma_max = 0 - the projection is not determined by the data;
 *          4 a non-finite value in this element's P or conf. out (and sv) are written in every case.
 * One deliberate difference from the reference: all arithmetic is float64 from the first load on (the reference forms L in float32, then widens).
 * One workgroup per batch element, L and its square in LDS, every product element one FMA chain over ascending k: bitwise reproducible,
 * independent of B, no atomics, no allocation, no host synchronisation (graph-capturable). One launch.
 * FORGE_ESHAPE unless 3 <= N <= 8 and N - 1 <= E <= N (N - 1) / 2; FORGE_EINVAL for a null pointer other than sv, B < 1, squares outside
 * 1..16, center outside 0..N-1, rank_tol outside [0, 1).
 */
int forge_pose_sync(const float* P, const float* conf, const int* pairs, int B, int N, int E, int squares, int center, double rank_tol,
                    float* out, double* sv, int* status, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g1  Triangle-mesh extraction from density volumes: marching tetrahedra on the Kuhn 6-tetrahedron split of every cell. The reference has no
 * geometry export; the field and the frame are the ray-marcher's (forge_render_fwd: align_corners=True sampling with zero padding).
 *   density  [n][D][H][W] float32, the plane of the [n,1,D,H,W] tensor of encoder_3d.get_density3D
 *   features [n][D][H][W][C] channels-last, nullable; C % 4 == 0, 16-byte aligned
 *   level    finite and > 0; a grid point is INSIDE iff d > level (strict, an fp32 compare)
 * Grid points have indices -1 .. N per axis; -1 and N are virtual zeros (and so is everything beyond them), which closes every surface, also one
 * that reaches the volume border. Cells have their min corner p0 in -1 .. N-1 per axis: (D+1)(H+1)(W+1) cells, linear index z-major
 * ((cz (H+1) + cy) (W+1) + cx with c = p0 + 1). Corner offset code: bit 0 = +x (W), bit 1 = +y (H), bit 2 = +z (D). Each cell is split into the six
 * tetrahedra p0, p0+e_a, p0+e_a+e_b, p0+(1,1,1) over the permutations (a,b,c) of (x,y,z) in lexicographic order. Every edge runs from a point to
 * that point plus a non-zero offset code and is OWNED by the cell whose min corner is its first point: edge direction k = 0..6 is offset code k+1.
 *   vertices one per ACTIVE edge (one end inside, one outside), welded. With a the inside end: t = (level - d_a) / (d_b - d_a) in fp32, index
 *            position idx = a + t (b - a), world position per axis ((2 idx) / (N-1) - 1) e, e = 0.5 (N-1) volume_size / N (fp32, this order;
 *            N-1 is replaced by 1 where N = 1). Emitted as (x, y, z) <-> (W, H, D): the canonical world frame forge_render_fwd takes cameras in.
 *   normals  -normalize(g_a + t (g_b - g_a)), g the central difference of the zero-padded field at a grid point scaled to world units
 *            (per axis (f(p+1) - f(p-1)) N: the common factor 2 volume_size drops out); a zero vector stays zero. They point to the low-density side.
 *   vertex_features  f_a + t (f_b - f_a), virtual points = 0 (only with features)
 *   order    vertices by (volume, owner cell linear index, edge direction); triangles by (volume, cell linear index, tetrahedron 0..5, triangle
 *            0..1); vertex indices are per volume; triangles are counter-clockwise seen from the low-density side. No atomics: the order, and
 *            every bit of the output, is reproducible. Every undirected edge of the result is shared by exactly two oppositely directed triangles.
 *
 *   forge_mesh_case_table    host only, no device: copies the case table (the ONE copy, a constexpr table in mesh.hip) into table[154]:
 *                            tet_corner[6][4] offset codes | tet_flip[6] (1: the path is negatively oriented, its triangles swap their last two
 *                            vertices) | tet_edge[6][2] local corner pairs i < j | case_ntri[16] | case_tri[16][2][3] tetrahedron-edge ids, for a
 *                            positively oriented tetrahedron, case = sum of 2^i over the inside local corners.
 *   forge_mesh_workspace_bytes  bytes of the workspace (16-byte aligned) shared by the two calls below; negative FORGE_E* for bad extents.
 *   forge_mesh_count         classify every cell, scan: counts[v] = (vertices, triangles) of volume v (device int32 [n][2]), the workspace holds the
 *                            cell records and offsets that forge_mesh_emit reads. Three launches.
 *   forge_mesh_emit          writes the mesh. offsets == NULL: volume v owns rows v max_vertices .. (v+1) max_vertices - 1 of vertices / normals /
 *                            vertex_features and rows v max_faces .. of faces. offsets != NULL (device int32 [n][2], the exclusive scan of counts
 *                            over volumes): volume v starts at row offsets[v] of arrays with max_vertices / max_faces rows IN ALL. Rows past
 *                            the capacity are never written; status[v] (device int32) = FORGE_MESH_OVERFLOW when volume v did not fit, else 0;
 *                            the rows that did fit are the prefix of the full result. A NEGATIVE offsets[v][0] or offsets[v][1] is never followed: volume v
 *                            writes nothing, to any array, and reports FORGE_MESH_OVERFLOW if it had anything to emit. Two launches.
 * Nothing allocates, synchronises or reads the environment: both calls may sit in a captured graph.
 * FORGE_EINVAL: null pointer, level <= 0 or not finite, volume_size <= 0 or not finite, an extent or n < 1, a workspace too small or unaligned,
 * negative capacities. FORGE_ESHAPE: C % 4 != 0, more than (2^31 - 1) / 12 cells per volume (per-volume offsets are 32-bit), n > 65535.
 */
#define FORGE_MESH_OVERFLOW 1   /* status bit of forge_mesh_emit: the volume's vertices or triangles exceed the capacity */
#define FORGE_MESH_TABLE_INTS 154
int forge_mesh_case_table(int* table, int capacity);
long long forge_mesh_workspace_bytes(int n, int D, int H, int W);
int forge_mesh_count(const float* density, int n, int D, int H, int W, float level, void* workspace, long long workspace_bytes, int* counts,
                     forge_stream_t stream);
int forge_mesh_emit(const float* density, const float* features, int n, int C, int D, int H, int W, float level, float volume_size,
                    const void* workspace, long long workspace_bytes, const int* counts, const int* offsets, int max_vertices, int max_faces,
                    float* vertices, float* normals, int* faces, float* vertex_features, int* status, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g2  Vertex colours for the meshes of g1, baked from posed images with a visibility test (csrc/bake.hip). A vertex is visible from a camera if
 * transmittance stays high along the segment from the vertex to the camera centre, through the field the ray-marcher and the mesh use
 * (align_corners=True trilinear sampling with zero padding): no depth maps, no rasteriser, no atomics. The reference has no counterpart.
 *   vertices, normals  the rows forge_mesh_emit wrote; counts [n][2], offsets [n][2] (nullable) and max_vertices select the same two row layouts:
 *                      offsets == NULL: volume k owns rows k max_vertices .. (k+1) max_vertices - 1; otherwise volume k starts at row offsets[k][0]
 *                      of arrays with max_vertices rows IN ALL. Volume k has min(counts[k][0], rows left to it) rows: a volume that overflowed bakes
 *                      the prefix that fitted. Rows past that are never written. A negative offsets[k][0] or offsets[k][1] is never followed: volume k
 *                      has no rows, nothing of it is read or written (as in g1 and g3).
 *   density  [n][D][H][W]; hx, hy, hz the half extents of W, H, D as forge_render_fwd takes them (finite, > 0)
 *   images   [V][C][Hi][Wi] planar, C in 1 .. 4; view_weight [V][Hi][Wi], nullable (= 1): a per-pixel confidence or foreground map
 *   cam      [V][16]: R[9] row-major (OpenCV world->camera, x_cam = R p + T), T[3], fx, fy, cx, cy in pixels OF THE GIVEN IMAGES (not the
 *            renderer's half resolution); the ray through pixel (h, w) is the renderer's, ((w+.5-cx)/fx, (h+.5-cy)/fy, 1)
 *   view2vol [V] the volume view v depicts; a vertex of volume k looks at the views with view2vol == k, in increasing v; a view whose index is
 *            outside 0 .. n-1 is ignored (a device-side compare, no read-back);  view_gain [V], nullable (= 1)
 *   colors [rows][C], weight [rows], best [rows] (int32), the rows laid out as vertices
 * For vertex p with normal nh, in a view v of its volume (all arithmetic fp32):
 *   projection     x_cam = R p + T; (x, y) = (fx x_cam.x / x_cam.z + cx - 0.5, fy x_cam.y / x_cam.z + cy - 0.5); IN VIEW iff x_cam.z >= z_near,
 *                  0 <= x <= Wi-1 and 0 <= y <= Hi-1. Colour c_v (per channel) and map value m_v: bilinear at (x, y), i0 = floor, the far tap
 *                  index clamped to the last row / column (its weight is 0 there), w00 I00 + w01 I01 + w10 I10 + w11 I11 in this order with
 *                  w00 = (1-ax)(1-ay), w01 = ax (1-ay), w10 = (1-ax) ay, w11 = ax ay.
 *   facing         c = -R^T T, dist = |c - p|, u = (c - p) / dist; max(0, nh.u)^cos_power by repeated multiplication; a zero normal: 1.
 *   transmittance  p0 = p + offset nh (p for a zero normal); for s = 0 .. S-1, t_s = (s + 0.5) step: a_s = clamp(d(p0 + t_s u), 0, 1) if t_s < dist,
 *                  else 0, with d the trilinear zero-padded sample at pix = ((pos / (hx,hy,hz) + 1) / 2) (N - 1) per axis, as in forge_render_fwd.
 *                  T_v = prod_s (1 - a_s), combined in a FIXED order: the eight partial products over s = j (mod 8), each in increasing s,
 *                  then pairwise j ^ 1, j ^ 2, j ^ 4. Samples with no tap inside the volume are exact factors of 1.
 *   weight         w_v = view_gain[v] m_v T_v facing (left to right) when in view, else 0.
 * Per row: weight = sum_v w_v in increasing v; best = the v of the largest w_v (ties: the lowest v; -1 if no w_v > 0); colors = (sum_v w_v c_v,
 * an fma chain in increasing v) / weight with mode 0, c_best with mode 1; where best = -1 or weight < w_min, colors = fill in every channel.
 * One launch; nothing allocates, synchronises or reads the environment (graph-capturable); every bit is reproducible. max_vertices = 0: no launch,
 * returns 0.
 * FORGE_EINVAL: a null pointer (offsets, view_weight, view_gain excepted), an extent, n or V < 1, S < 1, step or a half extent not finite or
 * <= 0, z_near not finite or <= 0, cos_power outside 1 .. 8, mode outside {0, 1}, offset or w_min negative or not finite, max_vertices < 0.
 * FORGE_ESHAPE: C outside 1 .. 4, D H W or Hi Wi or (offsets == NULL) n max_vertices beyond 2^31 - 1, n > 65535.
 */
int forge_mesh_bake(const float* vertices, const float* normals, const int* counts, const int* offsets, int n, int max_vertices,
                    const float* density, int D, int H, int W, float hx, float hy, float hz, const float* images, const float* view_weight,
                    int C, int Hi, int Wi, const float* cam, const int* view2vol, const float* view_gain, int V, int S, float step, float offset,
                    int cos_power, float z_near, float w_min, int mode, float fill, float* colors, float* weight, int* best, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g3  Scoring a surface against ground truth (csrc/geomdist.hip): deterministic surface samples of triangle meshes, exact nearest neighbours
 * between two point sets, and their reduction to accuracy / completeness / Chamfer / Hausdorff / F-score / normal consistency. The reference has
 * no counterpart. Brute force on purpose: exact, no build step, no data-dependent memory, no atomics, graph-capturable.
 *
 * forge_surface_sample  n_samples area-proportional points on each of n_mesh meshes, in the two row layouts of forge_mesh_emit:
 *   vertices, faces, counts [n_mesh][2], offsets [n_mesh][2] (nullable), max_vertices, max_faces  as g1 / g2 take them: offsets == NULL: mesh v owns
 *             rows v max_vertices .. of vertices and v max_faces .. of faces; otherwise mesh v starts at rows offsets[v] of arrays with max_vertices /
 *             max_faces rows IN ALL. Mesh v has min(counts[v], rows left to it) vertices and faces (count_v vertices below). counts stays on the device.
 *   area      A_f = 0.5 |cross(b - a, c - a)| of the fp32 corners a, b, c, evaluated in float64. A face with an index outside 0 .. count_v - 1 has
 *             area 0 and is never followed.
 *   cum       workspace[face row] (float64) = the inclusive sum of A_f over the mesh's faces, in a fixed order: with chunk = ceil(F / 256), the sum
 *             of the chunks before the face's own (chunk sums added in increasing chunk index, each formed in increasing f) plus the running sum
 *             within its chunk. A_total = cum[F - 1].
 *   sample i  u_i = (i + 0.5) / n_samples A_total (float64, left to right); face = the first f with cum[f] > u_i (binary search). Systematic
 *             sampling: face indices are non-decreasing in i, face f receives floor or ceil of n_samples A_f / A_total samples, a face of area 0
 *             receives none.
 *   bary      integers only: k1 = uint32(i 3242174889) >> 8, k2 = uint32(i 2447445414) >> 8 (the R2 sequence in 32-bit wrap-around arithmetic);
 *             if k1 + k2 > 2^24: k1 = 2^24 - k1, k2 = 2^24 - k2; r1 = k1 2^-24, r2 = k2 2^-24: exact in fp32, r1, r2 >= 0, r1 + r2 <= 1.
 *   points    [n_mesh][n_samples][3] = fma(r2, c - a, fma(r1, b - a, a)) per axis (fp32)
 *   normals   [n_mesh][n_samples][3] = normalize(cross(b - a, c - a)) in fp32 (components fma(e1y, e2z, -(e1z e2y)), ...): the face normal along
 *             the mesh's winding - outward for the meshes of g1; zero when the cross product is zero
 *   face      [n_mesh][n_samples] int32;  bary [n_mesh][n_samples][2] = (r1, r2)
 *   status    [n_mesh] int32: FORGE_GEOM_EMPTY when A_total is 0 or not finite; then points and normals are zero and face is -1 (bary is written
 *             all the same: it does not depend on the mesh).
 *   workspace forge_surface_sample_workspace_bytes(n_mesh, max_faces, packed = offsets != NULL) bytes, 16-byte aligned.
 *   Two launches. FORGE_EINVAL: a null pointer (offsets excepted; vertices / faces may be null with a zero capacity), n_mesh or n_samples < 1, a
 *   negative capacity, a workspace too small or unaligned. FORGE_ESHAPE: n_mesh > 65535, vertex / face / sample rows beyond 2^31 - 1.
 *
 * forge_nn_points  for each of B pairs and each query, the nearest reference:
 *   q [B][Nq][3], p [B][Np][3] fp32; q_count [B], p_count [B] device int32, nullable (= Nq, Np), clamped into 0 .. N
 *   xf [B][12], nullable: a row-major 3x4 (s R | t) applied to the QUERIES on load, x' = fma(m02, z, fma(m01, y, fma(m00, x, t0))) per row
 *   d2 [B][Nq] fp32 = min over j < p_count of fma(dz, dz, fma(dy, dy, dx dx)) with dx = q'.x - p_j.x etc. in fp32;  idx [B][Nq] int32 = that j.
 *   q_xf [B][Nq][3], nullable: the queries as they were scored (q' for every row, valid or not) - the references of the opposite direction.
 *   Ties go to the LOWEST reference index. Rows at or past q_count: d2 = 0, idx = -1. p_count = 0: d2 = +inf, idx = -1. A candidate wins only
 *   through `d2_j < best` (best starts at +inf), so a NaN coordinate never wins; a query with no winning reference at all keeps d2 = +inf, idx = -1.
 *   The DIFFERENCE form is deliberate, and not |q|^2 + |p|^2 - 2 q.p on the matrix cores: between two samplings of nearly the same surface - the
 *   regime the metric exists to measure - d2 ~ 1e-6 stands against terms ~ 0.25, and the expanded form cancels to nothing in fp32, while the
 *   difference form keeps a relative error of a few 2^-24 at any distance.
 *   One launch, grid (query blocks of forge_nn_queries_per_block(), pairs), references walked in LDS tiles of forge_nn_tile_points(); no split over
 *   the references, so no merge. FORGE_EINVAL: null q / p / d2 / idx, B, Nq or Np < 1. FORGE_ESHAPE: B > 65535, Nq or Np within a tile of 2^31.
 *
 * forge_geom_metrics  the distances of both directions reduced per pair, float64 throughout, d = sqrt((double)d2):
 *   d2_ab, idx_ab [B][Na] (queries A against references B), d2_ba, idx_ba [B][Nb]; normals_a [B][Na][3], normals_b [B][Nb][3]: both or neither;
 *   a_count, b_count [B] nullable as above; tau: n_tau <= FORGE_GEOM_MAX_THRESHOLDS finite thresholds, a HOST array read before the launch.
 *   Per direction over the count's valid rows: mean d, mean d2, max d, the fraction with d < tau_k, and the mean of |n_from[i] . n_to[idx[i]]| (an
 *   fma chain z, y, x in float64; rows with idx = -1 add 0). Per-workgroup partials (fixed tree) are summed in workgroup order by the second launch.
 *   out [B][FORGE_GEOM_OUT_DOUBLES]: ACCURACY = mean d of A -> B, COMPLETENESS = mean d of B -> A, CHAMFER_L1 = their mean, CHAMFER_L2 = the sum of
 *   the two mean d2, HAUSDORFF = the larger max, NORMAL_CONSISTENCY = the mean of the two directions (NaN without normals), then per threshold k
 *   PRECISION + k (A -> B), RECALL + k (B -> A), FSCORE + k = 2 P R / (P + R), 0 when P + R = 0 (NaN for k >= n_tau).
 *   status [B]: FORGE_GEOM_EMPTY when either count is 0; the means of an empty side are NaN (0 / 0) - never a trap, never a host check.
 *   partial: forge_geom_metrics_partial_doubles(B) doubles. Two launches.
 *   FORGE_EINVAL: a null pointer (normals, counts excepted; tau with n_tau = 0), normals of one side only, B, Na or Nb < 1, n_tau outside 0 .. 4, a
 *   threshold that is not finite, partial or out not 8-byte aligned. FORGE_ESHAPE: B > 65535.
 * Nothing allocates, synchronises or reads the environment; every entry takes the stream; every output bit is reproducible.
 */
#define FORGE_GEOM_EMPTY 1              /* status bit: a mesh without area (forge_surface_sample), a pair with an empty side (forge_geom_metrics) */
#define FORGE_GEOM_MAX_THRESHOLDS 4
#define FORGE_GEOM_ACCURACY 0
#define FORGE_GEOM_COMPLETENESS 1
#define FORGE_GEOM_CHAMFER_L1 2
#define FORGE_GEOM_CHAMFER_L2 3
#define FORGE_GEOM_HAUSDORFF 4
#define FORGE_GEOM_NORMAL_CONSISTENCY 5
#define FORGE_GEOM_PRECISION 6
#define FORGE_GEOM_RECALL 10
#define FORGE_GEOM_FSCORE 14
#define FORGE_GEOM_OUT_DOUBLES 18
int forge_nn_queries_per_block(void);
int forge_nn_tile_points(void);
int forge_geom_scan_threads(void);
long long forge_surface_sample_workspace_bytes(int n_mesh, int max_faces, int packed);
int forge_surface_sample(const float* vertices, const int* faces, const int* counts, const int* offsets, int n_mesh, int max_vertices, int max_faces,
                         int n_samples, void* workspace, long long workspace_bytes, float* points, float* normals, int* face, float* bary,
                         int* status, forge_stream_t stream);
int forge_nn_points(const float* q, const float* p, const int* q_count, const int* p_count, const float* xf, int B, int Nq, int Np, float* d2,
                    int* idx, float* q_xf, forge_stream_t stream);
long long forge_geom_metrics_partial_doubles(int B);
int forge_geom_metrics(const float* d2_ab, const int* idx_ab, const float* d2_ba, const int* idx_ba, const float* normals_a, const float* normals_b,
                       const int* a_count, const int* b_count, int B, int Na, int Nb, const double* tau, int n_tau, double* partial, double* out,
                       int* status, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g3b  Scoring samples against TRIANGLES (csrc/tridist.hip; the reduction in csrc/geomdist.hip): the distance from a point to a surface, not to
 * a sampling of it. Between two samplings of n points of a surface of area A the nearest sample lies about 0.5 sqrt(A / n) away however good the
 * reconstruction is; against the other side's triangles a mesh scored against itself gives 0 at any n. Brute force, as forge_nn_points.
 *
 * forge_nn_triangles  for each of B pairs and each query, the closest triangle of mesh b:
 *   q [B][Nq][3] fp32; q_count [B] device int32, nullable (= Nq), clamped into 0 .. Nq; xf_q [B][12], nullable: applied to the QUERIES on load by
 *             forge_nn_points' chain, x' = fma(m02, z, fma(m01, y, fma(m00, x, t0))) per row.
 *   vertices, faces, counts [B][2], offsets [B][2] (nullable), max_vertices, max_faces  the arrays forge_surface_sample takes, in both layouts.
 *   xf_mesh [B][12], nullable: applied to every VERTEX on load by the same chain - the mesh brought into the frame the queries are scored in.
 *   candidates  every face of mesh b except: a face with an index outside 0 .. count_v - 1, and a face whose area A_f (forge_surface_sample's:
 *             float64, from the fp32 corners BEFORE xf_mesh) is 0. Faces are taken in increasing index.
 *   arithmetic  all fp32, in this order. A = a - q', B = b - q', C = c - q' per component (a, b, c the transformed corners); everything after
 *             that is computed on A, B, C alone. ab = B - A, ac = C - A; with dot(u, v) = fma(uz, vz, fma(uy, vy, ux vx)):
 *               n1 = dot(ab, A), n2 = dot(ac, A), n3 = dot(ab, B), n4 = dot(ac, B), n5 = dot(ab, C), n6 = dot(ac, C)
 *               vc = fma(n1, n4, -(n3 n2)), vb = fma(n5, n2, -(n1 n6)), va = fma(n3, n6, -(n5 n4)), t34 = n3 - n4, t65 = n6 - n5
 *             (n_k = -d_k of Ericson, Real-Time Collision Detection 5.1.5: the query is the origin). The Voronoi region of the triangle that
 *             holds the query is the FIRST of these whose test holds, and it sets (vn, wn, den):
 *               vertex A   n1 >= 0 and n2 >= 0                  (0, 0, 1)
 *               vertex B   n3 <= 0 and n4 >= n3                 (1, 0, 1)
 *               edge AB    vc <= 0 and n1 <= 0 and n3 >= 0      (n1, 0, n1 - n3)
 *               vertex C   n6 <= 0 and n5 >= n6                 (0, 1, 1)
 *               edge AC    vb <= 0 and n2 <= 0 and n6 >= 0      (0, n2, n2 - n6)
 *               edge BC    va <= 0 and t34 >= 0 and t65 >= 0    (t65, t34, t34 + t65)
 *               interior   otherwise                            (vb, vc, (va + vb) + vc)
 *             r = 1 / den (ONE reciprocal on every path; the device's is within 1 ulp), v = vn r, w = wn r, and the closest point relative to
 *             the query is P = fma(w, ac, fma(v, ab, A)) per component; d2_f = fma(Pz, Pz, fma(Py, Py, Px Px)). Evaluated with selects, no
 *             branch; a NaN fails every test, takes the interior row and gives d2_f = NaN. No plane-distance formula and no |q|^2 + ...
 *             expansion: the closest-point form keeps the error of the barycentrics second-order in the distance.
 *   d2 [B][Nq] fp32 = min over the candidates of d2_f;  face [B][Nq] int32 = that f, relative to the mesh's first face row.
 *   closest [B][Nq][3], nullable: q' + P of the winning face per component - the closest point, in the frame the queries were scored in.
 *   normal [B][Nq][3], nullable: the unit normal of the winning face along its winding, forge_surface_sample's fp32 expression on the
 *             (transformed) corners: without xf_mesh, bit for bit the normal sample_surface gives for that face.
 *   A candidate wins only through `d2_f < best` (best starts at +inf): NaN never wins, ties go to the LOWEST face index. Rows at or past
 *   q_count: d2 = 0, face = -1. A query with no winning face (no candidates, a NaN query): d2 = +inf, face = -1. closest and normal are zero
 *   wherever face = -1.
 *   workspace forge_nn_triangles_workspace_bytes(B, max_faces, packed = offsets != NULL) bytes, 16-byte aligned: one record of 12 floats per
 *   face row (corners and normal; NaN for a face that is no candidate), written by a staging launch. Two launches: staging, then the search
 *   with grid (query blocks of forge_nn_queries_per_block(), pairs), records walked in LDS tiles of forge_nn_tile_faces(); no split over the
 *   faces, so no merge. FORGE_EINVAL: null q / counts / workspace / d2 / face (vertices / faces may be null with a zero capacity), B or Nq < 1,
 *   a negative capacity, a workspace too small or unaligned. FORGE_ESHAPE: B > 65535, vertex or face rows beyond 2^31 - 1, Nq or max_faces
 *   within a tile of 2^31.
 *
 * forge_geom_metrics_hits  forge_geom_metrics with ROW-ALIGNED "to" normals: hit_ab [B][Na][3] and hit_ba [B][Nb][3] (forge_nn_triangles'
 *   `normal`) in place of idx_ab / idx_ba. The normal term of row i is |n_from[i] . hit[i]|, the same float64 fma chain z, y, x; a zero hit
 *   adds 0. normals_a, hit_ab, normals_b, hit_ba: all four or none (NORMAL_CONSISTENCY is then NaN). Same outputs, partials, thresholds, status,
 *   launches and errors as forge_geom_metrics; d2 of either direction may come from forge_nn_points or forge_nn_triangles.
 * Nothing allocates, synchronises, reads the environment or uses atomics; every entry takes the stream; every output bit is reproducible.
 */
int forge_nn_tile_faces(void);
long long forge_nn_triangles_workspace_bytes(int n_mesh, int max_faces, int packed);
int forge_nn_triangles(const float* q, const int* q_count, const float* xf_q, const float* vertices, const int* faces, const int* counts,
                       const int* offsets, const float* xf_mesh, int B, int Nq, int max_vertices, int max_faces, void* workspace,
                       long long workspace_bytes, float* d2, int* face, float* closest, float* normal, forge_stream_t stream);
int forge_geom_metrics_hits(const float* d2_ab, const float* hit_ab, const float* d2_ba, const float* hit_ba, const float* normals_a,
                            const float* normals_b, const int* a_count, const int* b_count, int B, int Na, int Nb, const double* tau, int n_tau,
                            double* partial, double* out, int* status, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g3c  Inside or outside (csrc/winding.hip): the generalized winding number of a point with respect to a triangle mesh - the sum of the signed
 * solid angles of its triangles over 4 pi. For a closed mesh wound as g1 winds it, it is 1 inside and 0 outside; for a mesh with holes, or any
 * triangle soup, it stays near 1 inside and near 0 outside and crosses the holes smoothly, where ray parity has no answer. Brute force over
 * (query, face) pairs, as forge_nn_triangles.
 *
 * forge_winding_number  for each of B pairs and each query, w of mesh b:
 *   q, q_count, xf_q, vertices, faces, counts, offsets, xf_mesh, B, Nq, max_vertices, max_faces, workspace  forge_nn_triangles' arguments, word for
 *             word: both row layouts, q_count clamped into 0 .. Nq, xf_q applied to the queries and xf_mesh to every vertex on load by the chain
 *             x' = fma(m02, z, fma(m01, y, fma(m00, x, t0))), and the same candidates - every face of mesh b except a face with an index outside
 *             0 .. count_v - 1 and a face whose float64 area A_f of the fp32 corners BEFORE xf_mesh is 0. A face that is no candidate adds exactly 0.
 *   arithmetic  fp32, in this order. A = a - q', B = b - q', C = c - q' per component (a, b, c the transformed corners); with
 *             dot(u, v) = fma(uz, vz, fma(uy, vy, ux vx)) and sqrt the device's (v_sqrt_f32, within 1 ulp):
 *               la = sqrt(dot(A, A)), lb = sqrt(dot(B, B)), lc = sqrt(dot(C, C))
 *               n = B x C: nx = fma(By, Cz, -(Bz Cy)), ny = fma(Bz, Cx, -(Bx Cz)), nz = fma(Bx, Cy, -(By Cx));  num = dot(A, n)
 *               ab = dot(A, B), bc = dot(B, C), ca = dot(C, A);  den = fma(ca, lb, fma(bc, la, fma(ab, lc, (la lb) lc)))
 *               theta_f = atan2(num, den)       (Van Oosterom and Strackee: half the signed solid angle of the triangle seen from q')
 *             atan2(y, x) is written out, not a library's: ax = |x|, ay = |y|, mx = max(ax, ay), mn = min(ax, ay), t = mn (1 / mx) (ONE reciprocal,
 *             the device's, within 1 ulp), s = t t,
 *               p = 2.920691855e-03; p = fma(p, s, c) for c = -1.636792719e-02, 4.321185872e-02, -7.552213967e-02, 1.066600457e-01,
 *               -1.421105564e-01, 1.999377310e-01, -3.333315253e-01 in turn;  r = fma(p s, t, t)      (within 1.1 ulp of atan(t) on [0, 1])
 *               r = 1.57079637 - r if ay > ax;  r = 3.14159274 - r if x < 0;  atan2 = r with the sign of y.      Selects, no branch.
 *   terms that drop  a theta_f that is NaN adds 0 (one compare, one select): the NaN record of a face that is no candidate, a NaN corner, and a
 *             query ON a vertex, where num = den = 0 and t = 0 (1 / 0) = NaN - so atan2(0, 0) counts as 0. A NaN query gives w = 0.
 *   sum       faces in increasing index, in GROUPS of 8 consecutive faces counted from the mesh's first face: the 8 terms of a group are added
 *             in fp32, in order, starting from 0.f; each group total is widened and added to a float64 sum, in increasing group index;
 *             w = (float)(sum (1 / (2 pi))), the product in float64 with 1 / (2 pi) = 0.15915494309189535. The grouping is by face index, not by
 *             LDS tile. One running fp32 sum would grow its error with the face count; this keeps it at that of 8 terms.
 *   w [B][Nq] fp32: positive inside a mesh wound as g1 winds it (counter-clockwise seen from outside). Rows at or past q_count: 0. A mesh without
 *             candidates: 0.
 *   workspace forge_winding_workspace_bytes(B, max_faces, packed = offsets != NULL) bytes, 16-byte aligned: forge_nn_triangles' records, written by
 *   the same staging launch. Two launches: staging, then the sum with grid (query blocks of forge_nn_queries_per_block(), pairs), records walked
 *   in LDS tiles of forge_nn_tile_faces(); no split over the faces, no atomics, nothing read back. Every output bit is reproducible and independent
 *   of the pair's position in the batch and of padded versus packed rows. FORGE_EINVAL: null q / counts / workspace / w (vertices / faces may be
 *   null with a zero capacity), B or Nq < 1, a negative capacity, a workspace too small or unaligned. FORGE_ESHAPE: B > 65535, vertex or face rows
 *   beyond 2^31 - 1, Nq or max_faces within a tile of 2^31.
 */
long long forge_winding_workspace_bytes(int n_mesh, int max_faces, int packed);
int forge_winding_number(const float* q, const int* q_count, const float* xf_q, const float* vertices, const int* faces, const int* counts,
                         const int* offsets, const float* xf_mesh, int B, int Nq, int max_vertices, int max_faces, void* workspace,
                         long long workspace_bytes, float* w, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g4  Connected components of density volumes, and dropping the floaters (csrc/components.hip): which voxels belong to the object. A few-view
 * reconstruction emits the object plus small detached blobs; every stage of g1 - g3 pays for them. The reference has no counterpart.
 *   density  [n][D][H][W] float32, as in g1;  level finite and > 0; a voxel is INSIDE iff d > level (strict, an fp32 compare - the one g1 makes):
 *            NaN is outside, +inf is inside.
 *   adjacency  two inside voxels are neighbours iff their index difference (dx, dy, dz) is non-zero and has all three components in {0, +1} or all
 *            three in {0, -1}: 14 neighbours - the 6 axis neighbours, the three same-sign face diagonals, the same-sign body diagonal and their
 *            negatives; (+1, -1, 0) is NOT a neighbour. These are exactly the lattice edges g1 marches over (offset codes 1..7 of its case table).
 *            Nothing is adjacent across the volume border, across rows, or across the volumes of a batch.
 *   Why this adjacency: a component is then exactly one solid region of the surface of g1. Set the inside voxels of some components to zero and
 *   leave every other voxel as it is: no lattice edge joins a kept inside voxel to a removed one, so the mesh g1 extracts at any level >= this
 *   level is an ordered sub-mesh of the original - the same vertices bit for bit in the same relative order, the original faces filtered and
 *   re-indexed in the same order. (Normals may differ within two voxels of a removed voxel: the gradient stencil reads it.)
 *   labels   [n][D][H][W] int32: 0 outside, 1 .. K_v inside; the components of a volume are numbered by their LOWEST linear index
 *            (z H + y) W + x, ascending. Labels need no capacity.
 *   counts   [n] int32 = K_v
 *   statistics, integers, in label order, rows of capacity max_components (Kmax) per volume; rows at or past K_v are zero:
 *            sizes [n][Kmax] int32 voxel counts;  bbox [n][Kmax][6] int32 = x0, y0, z0, x1, y1, z1 inclusive;
 *            coord_sum [n][Kmax][3] int64 = the sums of the x, y, z indices (centroid = coord_sum / size, exact in the caller's float64);
 *            status [n] int32 = FORGE_COMPONENTS_OVERFLOW where K_v > Kmax: the rows are then the first Kmax components.
 *   selection  out [n][1][D][H][W] float32. With L_v the largest size in volume v, a component PASSES iff size >= min_voxels and
 *            size >= thr_v, thr_v = (int)ceil((double)min_fraction * (double)L_v): float64, L_v converts exactly, ONE rounding in the product,
 *            ceil exact. keep_largest = 0: every passing component is kept. keep_largest = 1: only one, the passing component of largest size,
 *            ties to the lowest label (it is the largest component of the volume, kept iff L_v >= min_voxels). out = the density's bits for
 *            outside voxels and for inside voxels of kept components (NaN payloads and signed zeros survive), +0.0f for inside voxels of removed
 *            components. A volume without inside voxels is copied. Selection needs no component capacity and no read-back: sizes live at the
 *            component's root voxel in the workspace.
 *
 *   forge_components_tile             host only: T, the edge of the cubic tile one workgroup labels in LDS (tile seams are where tests look).
 *   forge_components_workspace_bytes  bytes of the workspace (16-byte aligned) shared by the calls below; negative FORGE_E* for bad extents.
 *   forge_components_label   labels the volumes into the workspace, writes counts and, when labels != NULL, labels. Five launches, six with labels.
 *   forge_components_stats   after forge_components_label on the same workspace and extents: the statistics. Two launches. max_components = 0
 *                            writes status only (sizes, bbox, coord_sum may then be null).
 *   forge_components_select  after forge_components_label on the same workspace, extents and density: writes out. Two launches. out may not
 *                            alias density.
 * Union-find with parent[x] <= x, tile-local in LDS, then across tile faces by agent-scope fetch_min; every walk moves to a strictly smaller
 * index, no kernel waits for another workgroup. Integer atomics only (add, min, max on int32 / int64): every output bit is reproducible.
 * Nothing allocates, synchronises or reads the environment; every entry takes the stream and may sit in a captured graph.
 * FORGE_EINVAL: a null pointer (labels excepted), level <= 0 or not finite, an extent or n < 1, a workspace too small or unaligned,
 * max_components < 0, keep_largest outside {0, 1}, min_voxels < 1, min_fraction outside [0, 1] (NaN included).
 * FORGE_ESHAPE: D H W >= 2^31 - 1 (indices are 32-bit), n > 65535, n max_components > 2^31 - 1.
 */
#define FORGE_COMPONENTS_OVERFLOW 1   /* status bit of forge_components_stats: the volume has more components than max_components */
int forge_components_tile(void);
long long forge_components_workspace_bytes(int n, int D, int H, int W);
int forge_components_label(const float* density, int n, int D, int H, int W, float level, void* workspace, long long workspace_bytes, int* labels,
                           int* counts, forge_stream_t stream);
int forge_components_stats(const void* workspace, long long workspace_bytes, int n, int D, int H, int W, int max_components, int* sizes, int* bbox,
                           long long* coord_sum, int* status, forge_stream_t stream);
int forge_components_select(const float* density, int n, int D, int H, int W, void* workspace, long long workspace_bytes, int keep_largest,
                            int min_voxels, double min_fraction, float* out, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * g5  Aligning a prediction to ground truth (csrc/align.hip): the similarity q -> p that g3's `xf` takes, ESTIMATED - the closed-form least-squares
 * fit (Umeyama; Kabsch without scale) from float64 moments, as one update of an ICP whose correspondences are forge_nn_points', and the choice among
 * several starts. The reference has no counterpart. No atomics, no allocation, nothing read back; every output bit is reproducible and independent
 * of the batch; the rotation is csrc/so3.h's projection onto SO(3), U diag(1, 1, det) V^T - the one forge_pose_sync uses.
 *
 * forge_align_step  one update per pair, two launches:
 *   q [B][Nq][3], p [B][Np][3] fp32; q_count, p_count [B] device int32, nullable (= Nq, Np), clamped into 0 .. N as in g3
 *   idx [B][Nq] int32, nullable: row i of q matches row idx[i] of p; an idx outside 0 .. p_count - 1 skips the row and is never followed.
 *            Rows i < q_count are looked at. NULL: row i matches row i (known correspondences), rows i < min(q_count, p_count).
 *   d2  [B][Nq] fp32, nullable (NULL counts as 0): the squared distance of the match under the CURRENT transform (forge_nn_points' d2). Used for
 *            rejection and residuals only, never for the fit.
 *   state [B][FORGE_ALIGN_STATE_DOUBLES] float64, in and out:  T (12: row-major 3x4, s R | t, maps q to p) | SCALE s | RMSE | N_IN | N_VALID | CUT2 |
 *            DELTA | ITERATIONS | SV (3: singular values of H, descending) | SCORE | CQ (3) | CP (3): the centroids of the inliers' q and p
 *   xf [B][12] fp32, out: T rounded to nearest - the `xf` of the next forge_nn_points;   status [B] int32, in and out (bits below)
 *   host scalars: with_scale, update (0 or 1); reject, reject_floor, tol >= 0 and finite; rank_tol in [0, 1); clamp2 >= 0, may be +inf
 *   partial: forge_align_partial_doubles(B) doubles of work space.
 *   Launch 1, grid (forge_align_blocks(), B) x 256 threads, each striding over the rows. A row is VALID when it is matched and none of its six
 *   coordinates is infinite or NaN and its d2 is not NaN (else it is skipped and FORGE_ALIGN_NONFINITE is set); a valid row is an INLIER when
 *   !(d2 > CUT2), CUT2 from the incoming state. Values are widened to float64 on load. Per workgroup: n_in, n_valid, sum q (the RAW q, not the
 *   transformed one), sum p, sum p_r q_c (9: per thread acc = fma(p_r, q_c, acc) in row order), sum |q|^2 (fma(qz, qz, fma(qy, qy, qx qx)) per row) and
 *   sum d2 over the inliers, sum min(d2, clamp2) over the valid rows; each combined over the workgroup by ONE fixed tree (red[t] += red[t + s],
 *   s = 128 .. 1).
 *   The moments are those of the untransformed q: every step solves for the whole transform q -> p, so nothing is composed in fp32 and no error
 *   accumulates over the iterations of an ICP. One-pass raw moments suffice: coordinates are O(1) and n <= 2^20, so float64 leaves about
 *   n 2^-53 ~ 1e-10 absolute on sums whose centred values are about 0.05 n - nine digits of H survive the subtraction.
 *   Launch 2, one workgroup per pair: the partials are added in workgroup order, then one thread solves, every expression left to right:
 *     H_rc = sum p_r q_c - (sum p_r)(sum q_c) / n;  v_q = sum |q|^2 - |sum q|^2 / n  (n = n_in);  (R, SV) = projection of H onto SO(3)
 *     s = (sum_rc R_rc H_rc) / v_q with_scale and v_q > 0, else 1;  T = (s R | CP - s R CQ);  RMSE = sqrt(sum d2 / n_in);
 *     SCORE = sum min(d2, clamp2) / n_valid;  CUT2 = max(reject^2 sum d2 / n_in, reject_floor^2) for reject > 0, else +inf;
 *     DELTA = max |T_new - T_old| over the 12 entries (NaN if any is);  ITERATIONS += 1.
 *   RMSE, N_IN, N_VALID, SCORE, CQ and CP describe the INCOMING transform (they come from the incoming d2), T and SV the outgoing one.
 *   update = 0: statistics only - RMSE, N_IN, N_VALID, SCORE, CQ, CP are written, everything else stands (xf is rewritten from T).
 *   status: FORGE_ALIGN_EMPTY     n_in < 3: T, SCALE, SV and CUT2 are kept, DELTA = 0, and the pair does not count as converged
 *           FORGE_ALIGN_RANK      SV[1] / SV[0] < rank_tol or SV[0] = 0: the matched points are collinear; T is written all the same - a proper
 *                                 rotation that fits the line, its turn about the line arbitrary
 *           FORGE_ALIGN_NONFINITE a row was skipped for a non-finite value
 *           FORGE_ALIGN_CONVERGED DELTA <= tol
 *   update = 1 writes all four bits afresh; update = 0 keeps RANK and CONVERGED and writes the other two. A pair that ENTERS with CONVERGED set
 *   is frozen, whatever `update` is: neither launch reads its rows, state and status stand, xf is rewritten from T. Its RMSE, N_IN, N_VALID and
 *   SCORE therefore stay those of the step that converged, which describe the transform that came INTO that step: the final T itself when
 *   tol = 0 (DELTA = 0), a transform within tol per entry of it otherwise. forge_align_select compares such scores as they stand. The result of a loop of
 *   searches and steps is then a function of the inputs and the iteration budget alone - no host decision, so the loop can be captured.
 *   FORGE_EINVAL: a null q / p / partial / state / xf / status, B, Nq or Np < 1, with_scale or update outside {0, 1}, reject, reject_floor or tol
 *   negative or not finite, rank_tol outside [0, 1), clamp2 negative or NaN, partial or state not 8-byte aligned. FORGE_ESHAPE: B > 65535, Nq or
 *   Np within a launch's stride of 2^31.
 *
 * forge_align_select  state [B][K][FORGE_ALIGN_STATE_DOUBLES], status [B][K]: K starts per pair. best [B] int32 = the k of the lowest SCORE: the
 *   compare is a strict `<` in increasing k from +inf, so the lowest index wins a tie and NaN (and +inf) never wins; a start with EMPTY set never
 *   wins. T [B][4][4] float64 (bottom row 0 0 0 1), xf [B][12] fp32, state_out [B][FORGE_ALIGN_STATE_DOUBLES], status_out [B]: of the winner.
 *   best = -1 if none won: start 0 is then what is written. One launch.
 *   FORGE_EINVAL: a null pointer, B or K < 1, state, T or state_out not 8-byte aligned. FORGE_ESHAPE: B > 65535, B K beyond 32-bit rows.
 * Nothing allocates, synchronises or reads the environment; every entry takes the stream and may sit in a captured graph.
 */
#define FORGE_ALIGN_EMPTY 1
#define FORGE_ALIGN_RANK 2
#define FORGE_ALIGN_NONFINITE 4
#define FORGE_ALIGN_CONVERGED 8
#define FORGE_ALIGN_T 0
#define FORGE_ALIGN_SCALE 12
#define FORGE_ALIGN_RMSE 13
#define FORGE_ALIGN_N_IN 14
#define FORGE_ALIGN_N_VALID 15
#define FORGE_ALIGN_CUT2 16
#define FORGE_ALIGN_DELTA 17
#define FORGE_ALIGN_ITERATIONS 18
#define FORGE_ALIGN_SV 19
#define FORGE_ALIGN_SCORE 22
#define FORGE_ALIGN_CQ 23
#define FORGE_ALIGN_CP 26
#define FORGE_ALIGN_STATE_DOUBLES 29
int forge_align_blocks(void);
long long forge_align_partial_doubles(int B);
int forge_align_step(const float* q, const float* p, const int* q_count, const int* p_count, const int* idx, const float* d2, int B, int Nq, int Np,
                     int with_scale, int update, double reject, double reject_floor, double tol, double rank_tol, double clamp2, double* partial,
                     double* state, float* xf, int* status, forge_stream_t stream);
int forge_align_select(const double* state, const int* status, int B, int K, double* T, float* xf, int* best, double* state_out, int* status_out,
                       forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * h  Photographs to input tensors (csrc/ingest.hip): the `_load_frame` of dataset/kubric.py:410-445, dataset/gso.py:257-290 and
 * dataset/omniobject3d.py:221-258 and the image loop of demo.py:236-256 - an 8-bit RGB(A) frame of any size put on a background, resized with
 * Pillow's Image.ANTIALIAS (Lanczos, a = 3), its mask resized with Image.NEAREST, divided by 255. On 8-bit images Pillow's resampler is integer
 * arithmetic after the coefficient table, so the result is Pillow's bit for bit (tests/golden/ingest_pillow.npz), not to a tolerance.
 * Not covered: train.normalize_img (False in every configuration), the depth TIFFs of the Kubric loader, file decoding.
 *
 * One axis, n_in input and n_out output samples, float64 throughout:
 *   scale = n_in / n_out, fs = max(scale, 1), support = 3 fs. For output i: c = (i + 0.5) scale, first = max((int)(c - support + 0.5), 0),
 *   count = min((int)(c + support + 0.5), n_in) - first, w_j = L((j + first - c + 0.5) (1 / fs)) for j < count, with
 *   L(x) = sinc(x) sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, sinc(x) = sin(pi x) / (pi x). The w_j are divided by their sum (summed in
 *   increasing j) unless it is 0; k_j = (int)(w_j 2^22 + 0.5) for w_j >= 0, (int)(w_j 2^22 - 0.5) otherwise ((int) truncates).
 *   nearest: index_i = min((int)p_i, n_in - 1), p_0 = 0.5 scale, p_(i+1) = p_i + scale - the RUNNING float64 sum Pillow keeps, which differs
 *   from floor((i + 0.5) scale) where a tap lands on an integer (6 -> 9 samples, for one).
 * One pass over bytes: out = clamp((2^21 + sum_j k_j in[first + j]) >> 22, 0, 255), int32 accumulator, arithmetic shift, channels independent.
 * A resize is the horizontal pass (an 8-bit image H x Wo), then the vertical pass; Pillow skips a pass whose sizes agree, which the identity
 * table below reproduces.
 *
 *   forge_resample_taps     host only: K, the largest count of the axis (> 0), or FORGE_EINVAL for a non-positive size.
 *   forge_resample_coeffs   host only: first[n_out], count[n_out], k[n_out][K] with K = forge_resample_taps(n_in, n_out), rows zero-padded.
 *   forge_resample_nearest  host only: index[n_out].
 *   All three write host arrays, call nothing of the GPU runtime and allocate nothing. FORGE_EINVAL: a non-positive size, a null pointer.
 *
 *   forge_ingest_rgba8
 *   src      uint8 [N][H][W][C] on the device, C = 3 or 4, pixels packed; image_stride and row_stride in BYTES. Rows need no alignment.
 *   table_x, table_y  one DEVICE int32 table per axis, n = Wo resp. Ho, K = Kx resp. Ky:  first[n] | count[n] | nearest[n] | k[K][n]  - the
 *            coefficients TAP-MAJOR (k[j][i], the transpose of what forge_resample_coeffs writes). An axis whose sizes agree takes
 *            first = nearest = i, count = 1, k = 2^22, K = 1: a copy. The kernels clamp first / count / nearest into the source, so a wrong
 *            table gives wrong pixels, never an access outside src.
 *   background  0 black: the RGB bytes are resized with alpha ignored; images = bytes / 255 times the resized mask (dataset.mask_images = True)
 *               1 white: each channel is first put over white, t = c a + 255 (255 - a) + 128, (t + (t >> 8)) >> 8; not masked afterwards
 *               2 premasked: RGB is zeroed where alpha == 0, then resized; not masked afterwards (demo.py:244-248)
 *            With C = 3 there is no alpha: 1 and 2 resize the bytes as they are.
 *   workspace  N H Wo 4 bytes, 4-byte aligned: the intermediate, one packed pixel per dword.
 *   images   [N][3][Ho][Wo] float32: (float)byte / 255.0f, which is float32(float64(byte) / 255.0) for all 256 bytes; nullable
 *   masks    [N][1][Ho][Wo] float32, 0 or 1: the source mask at (nearest_y[y], nearest_x[x]); C = 4: alpha > 0; C = 3: (R > 0) | (G > 0) - blue
 *            plays no part: the third operand of np.logical_or at omniobject3d.py:228-230 is its `out=` argument; reproduced literally; nullable
 *   bytes    [N][Ho][Wo][3] uint8, Pillow's bytes; nullable
 * Two launches; nothing allocates, synchronises or uses atomics (graph-capturable).
 * FORGE_EINVAL: a null src / table / workspace, a non-positive dimension or K, C outside {3, 4}, an unknown background, row_stride < W C,
 * overlapping images, a workspace too small or unaligned. FORGE_ESHAPE: H row_stride, H Wo 4 or Ho Wo 3 beyond 2^31 - 1, or more workgroups
 * than one launch takes.
 */
int forge_resample_taps(int n_in, int n_out);
int forge_resample_coeffs(int n_in, int n_out, int* first, int* count, int* k);
int forge_resample_nearest(int n_in, int n_out, int* index);
int forge_ingest_rgba8(const unsigned char* src, int N, int H, int W, int C, long long image_stride, long long row_stride, const int* table_x, int Kx,
                       const int* table_y, int Ky, int Ho, int Wo, int background, void* workspace, long long workspace_bytes, float* images,
                       float* masks, unsigned char* bytes, forge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * layout helpers: NCDHW <-> channels-last for callers that hold plain-contiguous volumes.
 *   src [n][C][P] -> dst [n][P][C]   (P = D*H*W)   and back.
 */
int forge_ncdhw_to_ndhwc(const float* src, float* dst, int n, int C, long long P, forge_stream_t stream);
int forge_ndhwc_to_ncdhw(const float* src, float* dst, int n, int C, long long P, forge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FORGE_HIP_H */
