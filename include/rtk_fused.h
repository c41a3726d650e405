/*
 * rtk_fused.h -- C ABI of the fused inference stages of librtk_hip.so.
 *
 * These entry points have no single counterpart in the reference: each one replaces a SEQUENCE of
 * framework ops + pointnet2_cuda calls that the reference issues from Python, fused
 * into one gfx950 kernel working on point-major (row = point, contiguous channels) fp32 tensors:
 *
 *   rtk_pointwise_mlp   [three_nn weights + three_interpolate + cat skip] -> [Conv 1x1 + BN + act] x L
 *                       (lib/pointnet2_modules.py:140-158, lib/pytorch_utils.py:20-32,
 *                        utils/model_utils/model_utils.py:308-357, nn.Linear bottlenecks :414-418)
 *   rtk_sa_scale        group (xyz - centroid || features) -> SharedMLP -> max over the ball
 *                       (lib/pointnet2_utils.py:269-292 + lib/pointnet2_modules.py:37-53)
 *   rtk_cost_volume     kNN gather -> 3-layer MLP -> WeightNet -> weighted sum over neighbours
 *                       (utils/model_utils/model_utils.py:216-236)
 *   rtk_patch_cost      kNN gather -> WeightNet -> weighted sum          (model_utils.py:238-248)
 *
 * BatchNorm (eval mode) is folded into the packed weights/bias on the host; weights use the
 * fragment-major packing documented in ratrack_amd/csrc/fused_common.h.  Same conventions as
 * rtk_pointnet2.h: caller-allocated device buffers, explicit stream, 0 / negative status.
 */
#ifndef RTK_FUSED_H
#define RTK_FUSED_H

#include "rtk_pointnet2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTK_MAX_SRC 4
#define RTK_MAX_LAYERS 4

/* One input segment of a concatenated per-point feature vector. */
typedef struct {
    const float *ptr;  /* (rows, pitch) point-major, or (samples, pitch) when per_sample != 0 */
    int pitch;         /* floats per row, multiple of 4, buffer readable up to ceil4(channels) */
    int channels;      /* valid channels; the segment occupies ceil16(channels) input slots.  Columns channels .. ceil4(channels) are
                        * loaded with the last valid ones and enter the arithmetic (on the split path the position's scale too): they
                        * must hold ZERO, which is what rtk_prepare_inputs supplies for the raw (RCS, v_r, 0, 0) rows */
    int per_sample;    /* 1: row index = sample (broadcast over the sample's points) */
} rtk_src_t;

/* One 1x1-conv layer with folded BN: y = act(W x + b).  w_packed is [cin16][cout16][64][4] floats -- or, with RTK_LAYER_SPLIT
 * or-ed into act (rtk_pointwise_mlp only; all layers of a chain alike), the layer's 16-position split image: one 1 KiB fragment of
 * 64 lanes x 8 fp16 per (pair of 16-channel input blocks, 16-channel output block, piece h / l) of 2^k W, see csrc/fused_common.h,
 * with inv_scale = 2^-k (k: max|W| 2^k in [2^14, 2^15)). */
#define RTK_LAYER_SPLIT 0x100
typedef struct {
    const float *w_packed;
    const float *bias; /* 16*cout16 floats (zero padded) */
    int cin16, cout16; /* channel counts in units of 16 */
    int act;           /* RTK_ACT_* (0 none, 1 relu, 2 leaky 0.1, 3 sigmoid) */
    float inv_scale;   /* split images only: the inverse of the image's power-of-two weight scale */
} rtk_layer_t;

/* Optional first segment produced by three-NN inverse-distance interpolation. */
typedef struct {
    const float *known_feats; /* (samples * m, pitch) point-major */
    int pitch, channels, m;
    const int *idx;       /* (rows, 3) int32, indices into the sample's m known points */
    const float *dist2;   /* (rows, 3) squared distances from rtk_three_nn */
    const int *nuniq;     /* optional (samples): known rows >= nuniq[b] are duplicates of row 0 and read as row 0 */
} rtk_interp_t;

/* rows = total points (samples * rows_per_sample).  Input vector = [interp segment (optional)] ||
 * srcs[0] || srcs[1] ...; each segment padded to a multiple of 16 channels.  sample_bias (optional,
 * (samples, 16*layers[0].cout16)) is added to layer 0's pre-activation.  Output: point-major
 * (rows, out_pitch) at channel offset 0, or channel-major (samples, out_channels, rows_per_sample)
 * when out_channel_major != 0; only out_channels channels are written.
 * row_nuniq (optional, (samples)): rows r >= row_nuniq[b] of sample b are duplicates of the sample's row 0
 * (centroids picked after furthest-point sampling exhausted the cloud, see rtk_fps_centroids); they are
 * never written and never influence a result -- consumers alias them to row 0.  The kernel does load the source rows and the
 * interp.idx / interp.dist2 rows of such rows up to the end of the last live group of 64 rows (masked at the store): those buffers
 * must be readable for all `rows` rows, and the index rows must hold IN-RANGE indices (the three-NN kernels write whole groups).
 * colmax (optional, (samples, 16*last.cout16), ZERO-INITIALISED by the caller): per-sample maximum over the rows of
 * every output channel (torch.max(features, -1), models/track4d.py:89-92), accumulated with atomic max on the float
 * bits -- only valid when the last activation is non-negative (ReLU / sigmoid). */
RTK_EXPORT int rtk_pointwise_mlp(int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
                                 const rtk_src_t *srcs, const float *sample_bias, int nlayers,
                                 const rtk_layer_t *layers, float *out, int out_pitch, int out_channels,
                                 int out_channel_major, const int *row_nuniq, float *colmax, rtk_stream_t stream);

/* ... with the tile loop software-pipelined by one group: row_nuniq[b], interp.nuniq[b] and the first group's rows requested
 * together, the next group's rows requested under the current group's products and stores (only if that group is live).  Same
 * arguments, bit-identical result.  Measured in one build against the serial loop rtk_pointwise_mlp runs, it does not pay at the
 * benchmarked shapes; it is kept as the comparison implementation of the tests and of the same-box
 * measurements. */
RTK_EXPORT int rtk_pointwise_mlp_pipelined(int rows, int rows_per_sample, const rtk_interp_t *interp, int nsrc,
                                              const rtk_src_t *srcs, const float *sample_bias, int nlayers,
                                           const rtk_layer_t *layers, float *out, int out_pitch, int out_channels,
                                           int out_channel_major, const int *row_nuniq, float *colmax, rtk_stream_t stream);

/* rtk_pointwise_mlp of one split layer on a 128-channel interpolation segment (the encoder's fp1: split 128 -> 128 image, no other
 * source, no sample bias, every row live) writing out (rows, out_pitch) channels 0..127 and colmax exactly as rtk_pointwise_mlp does,
 * and then taking the same tile through one more split layer, 128 -> 256 without activation: proj_out[(rows, proj_pitch)] =
 * proj[k] applied to the layer's output, k = 0 for samples < frame_split and 1 for the others (the cost volume's first-layer
 * projections of frame 1 and frame 2, whose per-sample terms the cost volume adds: rtk_cost_volume_split_term).  Bit for bit what
 * rtk_pointwise_mlp gives for the layer alone and for proj[k] on its output. */
RTK_EXPORT int rtk_pointwise_mlp_tap(int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
                                     int out_pitch, float *colmax, const rtk_layer_t *proj, int frame_split, float *proj_out,
                                     int proj_pitch, rtk_stream_t stream);

/* ... with the software-pipelined tile loop: see rtk_pointwise_mlp_pipelined.  Same arguments, bit-identical result. */
RTK_EXPORT int rtk_pointwise_mlp_tap_pipelined(int rows, int rows_per_sample, const rtk_interp_t *interp, const rtk_layer_t *layer, float *out,
                                            int out_pitch, float *colmax, const rtk_layer_t *proj, int frame_split, float *proj_out,
                                            int proj_pitch, rtk_stream_t stream);

/* Two chains that read the same rows, in one launch: chain A (one split layer, 25 -> 2 blocks of 16 channels) on the whole input
 * vector srcs[0] || srcs[1] ... (25 slots) with its optional sample_bias, written point-major to out_a (rows, out_a_pitch); chain B
 * (four split layers, 16 -> 8 -> 4 -> 2 -> 1 blocks) on the last source alone (256 channels), written channel-major to out_b
 * (samples, out_b_channels, rows_per_sample).  The images lie in one blob, chain A's first: layers_b[0].w_packed follows layer_a's
 * image, and so on.  Every row is live.  Both outputs are bit for bit what rtk_pointwise_mlp gives for each chain on its own (the
 * decoder front: the sa1 projections of [raw | f1 | cor] and the class head on cor). */
RTK_EXPORT int rtk_pointwise_mlp_pair(int rows, int rows_per_sample, int nsrc, const rtk_src_t *srcs, const float *sample_bias,
                                      const rtk_layer_t *layer_a, float *out_a, int out_a_pitch, int out_a_channels, int nlayers_b,
                                      const rtk_layer_t *layers_b, float *out_b, int out_b_channels, rtk_stream_t stream);

/* One scale of a set-abstraction level.  q (samples*n, q_pitch): per-point layer-1 projection of the
 * features (BN scale folded); layer 1 = relu(q[idx] + Wx.(xyz[idx] - centroid) + b1) with
 * w1xyz_packed the [1][c1_16][64][4] image of [Wx | b1]; then nlayers more packed layers; the last
 * one's bias+ReLU is applied after the max over the nsample neighbours.  idx from rtk_ball_query.
 * out (samples*npoint, out_pitch) receives 16*last.cout16 channels at out_offset.
 * src_nuniq / dst_nuniq (optional, (samples)): duplicate-row counters of the source level (q rows >= src_nuniq[b]
 * are read as row 0) and of the centroid level (centroids >= dst_nuniq[b] are skipped: neither computed nor written).
 * What the entries may READ of those skipped centroids (this entry point and rtk_sa_scale_split; not the _serial ones): their
 * prologue requests the idx and new_xyz rows of every wave's first group of centroids before dst_nuniq[b] has arrived, so rows of
 * centroids in [dst_nuniq[b], npoint) may be loaded -- always inside the (samples, npoint) tables -- and are then discarded: no
 * address and no output value is formed from them, whatever they hold (uninitialised memory included).
 * Non-finite inputs (this entry point and rtk_sa_scale_split): the ReLU and the max over the neighbours follow IEEE maxNum and drop a
 * NaN (the reference propagates it), so an output can be finite where the reference's is NaN; it is never non-finite where the
 * reference's is finite.  The cost volume and patch cost below propagate: non-finite exactly where the reference is. */
RTK_EXPORT int rtk_sa_scale(int samples, int n, int npoint, int nsample, const float *xyz,
                            const float *new_xyz, const int *idx, const float *q, int q_pitch, int c1_16,
                            const float *w1xyz_packed, int nlayers, const rtk_layer_t *layers, float *out,
                            int out_pitch, int out_offset, const int *src_nuniq, const int *dst_nuniq,
                            rtk_stream_t stream);

/* rtk_sa_scale with the prologue and the tile loop as they were before the loop was software-pipelined (one unit's loads requested,
 * waited for and used before the next unit's go out; no row of a centroid >= dst_nuniq[b] is read).  Same arguments, bit-identical result; the comparison implementation of tests and timing tools,
 * not called by the package. */
RTK_EXPORT int rtk_sa_scale_serial(int samples, int n, int npoint, int nsample, const float *xyz,
                                   const float *new_xyz, const int *idx, const float *q, int q_pitch, int c1_16,
                                   const float *w1xyz_packed, int nlayers, const rtk_layer_t *layers, float *out,
                                   int out_pitch, int out_offset, const int *src_nuniq, const int *dst_nuniq,
                                   rtk_stream_t stream);

/* Point-to-patch cost volume for k = 16 neighbours.  p1 (samples*n1, 256) / p2 (samples*n2, 256):
 * first-layer projections of the query / neighbour features (bias folded into p1);
 * layer 1 = leaky(p1[i] + p2[idx] + Wd.(xyz2[idx] - xyz1[i])), then layers[0..1] (256->256, leaky),
 * WeightNet wn[0..2] (3->8->8->256, ReLU) on the same direction vectors, out = sum_k wn * feat. */
RTK_EXPORT int rtk_cost_volume(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                               const int64_t *knn_idx, const float *p1, const float *p2,
                               const float *wd_packed, const rtk_layer_t *layers,
                               const rtk_layer_t *wn, float *out, int out_pitch, rtk_stream_t stream);

/* Patch-to-patch aggregation: out[i] = sum_k WeightNet(xyz[idx[i,k]] - xyz[i]) * feat[idx[i,k]]. */
RTK_EXPORT int rtk_patch_cost(int samples, int n, const float *xyz, const int64_t *knn_idx,
                              const float *feat, int feat_pitch, const rtk_layer_t *wn, float *out,
                              int out_pitch, int out_channel_major, rtk_stream_t stream);
/* The same operator on the kernel with one wave per point (16 positions); rtk_patch_cost runs a 32-position tile (two points per
 * wave, csrc/fused_patch.hip) and hands the channel-major output, and feature buffers of 4 GiB and more, to this one.  Same
 * arguments, same contract, the same bits. */
RTK_EXPORT int rtk_patch_cost_wave16(int samples, int n, const float *xyz, const int64_t *knn_idx,
                                     const float *feat, int feat_pitch, const rtk_layer_t *wn, float *out,
                                     int out_pitch, int out_channel_major, rtk_stream_t stream);

/* ---- split matrix path (csrc/split_mfma.h): fp32 results from the fp16 matrix pipe --------------------------------------
 * Every fp32 operand, scaled by an exact power of two, is the sum of two fp16 pieces up to 2^-23 of itself; a product is the
 * three partial products l.h + h.l + h.h accumulated in fp32.  The error is that of an fp32 fmaf chain (2.7e-7 of max|y| on a
 * 256-deep product against float64; an fp32 GEMM: 6.4e-7); the matrix time is 3/16 of the fp32-input MFMA's, the only exact-fp32
 * matrix instruction of gfx950.  Scales: one power of two per weight matrix (chosen by the packer), one per position (chosen by
 * the kernels from the position's own largest activation) -- the path has no operand range to leave, inputs of any fp32
 * magnitude give fp32-accurate results.  A non-finite activation makes every output of its position non-finite (inf splits into an
 * inf and a NaN piece); the activations between layers (v_med3) map NaN to +inf (LeakyReLU) or 0 (ReLU): see rtk_sa_scale for what
 * reaches the outputs.
 *
 * rtk_pack_split_layer: w (cout, cin) row-major fp32 (transposed != 0: the layer is w^T, w stored (cin, cout) row-major -- the
 * backward's W^T products from the forward's weights), both multiples of 32, cout * cin <= 2^22 -> image of cin/16 * cout/32 * 2
 * fragments of 1 KiB (4 * cout * cin bytes), fragment (s, v, p) = piece p (0: h, 1: l) of 2^k W, rows 32 v .. +31 against the 16
 * input channels of k-step s in the lane order of v_mfma_f32_32x32x16_f16; *inv_scale = 2^-k (k: max|W| 2^k in [2^14, 2^15)).
 * Consumers take the image and a pointer to its inverse scale (layers back to back: images back to back, scales back to back).
 * rtk_split_mlp2: y = leaky(W2 leaky(W1 x + b1) + b2), LeakyReLU(0.1), x / y (positions, 256) point-major; images = the split
 * images of W1 and W2 back to back, image_scales = their two inverse scales.  The inner layers of the cost volume
 * (utils/model_utils/model_utils.py:216-236) as a standalone operator: what tests and tools time the matrix path with. */
RTK_EXPORT int rtk_pack_split_layer(int cout, int cin, const float *w, int transposed, void *image, float *inv_scale,
                                    rtk_stream_t stream);
/* rtk_cost_volume with its two 256 x 256 layers on the split path: same arguments, the layers as their split images (W2, W3
 * back to back, 2 * 262144 bytes, with their two inverse scales) and fp32 biases instead of the packed rtk_layer_t pair.  samples * n2 <= 2^22 (the gathered
 * p2 rows are requested with 32-bit byte offsets; RTK_ERR_INVALID beyond: split the batch). */
RTK_EXPORT int rtk_cost_volume_split(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                     const int64_t *knn_idx, const float *p1, const float *p2, const float *wd_packed,
                                     const void *split_images, const float *image_scales, const float *bias2,
                                     const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch, rtk_stream_t stream);
/* ... on a share of the chip.  The kernel keeps a CU whole (434 registers per lane, 144 KiB of LDS): launched with one workgroup per
 * CU it stops every other kernel for its duration.  With several batches in flight (ratrack_amd.fused.GraphPipeline) the step is
 * shorter when it takes `workgroups` < the CU count -- 3/4 of them at B = 64: the kernel itself runs 16 % longer, the pipelined
 * forward 2 % faster, the other batches' kernels keep a quarter of every XCD.  workgroups = 0: all CUs (rtk_cost_volume_split);
 * rounded down to a multiple of 8 (one share per XCD: all tiles of sample s run on XCD s % 8); ignored unless samples % 8 == 0. */
RTK_EXPORT int rtk_cost_volume_split_shared(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                            const int64_t *knn_idx, const float *p1, const float *p2, const float *wd_packed,
                                            const void *split_images, const float *image_scales, const float *bias2,
                                            const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch, int workgroups,
                                            rtk_stream_t stream);
/* rtk_cost_volume_split_shared as it was before the kernel kept its constants in LDS: layer 1's direction weights, the WeightNet's
 * layers and the biases are read from global memory on every tile.  Same arguments, bit-identical result; the comparison implementation
 * of tests and timing tools, not called by the package. */
RTK_EXPORT int rtk_cost_volume_split_gconst(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                            const int64_t *knn_idx, const float *p1, const float *p2, const float *wd_packed,
                                            const void *split_images, const float *image_scales, const float *bias2,
                                            const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch, int workgroups,
                                            rtk_stream_t stream);
/* ... with layer 1's per-sample term moved out of p1: sample_term (samples, 256) is added to the p1 row of every point of its sample
 * before the neighbour's p2 row, layer 1 = leaky((p1[i] + sample_term[b]) + p2[idx] + Wd.d), each sum rounded to fp32 -- bit for bit
 * rtk_cost_volume_split_shared on p1 + sample_term[b].  (p1, p2 without their per-sample terms: rtk_pointwise_mlp_tap.) */
RTK_EXPORT int rtk_cost_volume_split_term(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                          const int64_t *knn_idx, const float *p1, const float *p2, const float *sample_term,
                                          const float *wd_packed, const void *split_images, const float *image_scales,
                                          const float *bias2, const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch,
                                          int workgroups, rtk_stream_t stream);
/* The forward cost volume on a 16-position tile (one query point per wave, eight waves per workgroup, two per SIMD;
 * v_mfma_f32_16x16x32_f16): the same operator on the same arithmetic pieces as rtk_cost_volume_split_shared / _term -- the same split
 * pieces under the same per-position scales, fp32 accumulation; the bits differ because a matrix instruction sums 32 products instead
 * of 16, and the WeightNet's output layer its 8 in another order.  Same arguments and limits, but the two layers come in the
 * fragment order of the 16-position tile:
 * rtk_pack_split_layer16: as rtk_pack_split_layer (same scale, same pieces), image of cin/32 * cout/16 * 2 fragments of 1 KiB,
 * fragment (up, v, p) = piece p of 2^k W, rows 16 v .. +15 against the 32 input channels of k-step up; lane 16 g + i holds
 * W[16 v + i][32 up + 16 (t / 4) + 4 g + t % 4], t = 0..7 (ratrack_amd.fused.pack_layer_split16 is its host restatement). */
RTK_EXPORT int rtk_pack_split_layer16(int cout, int cin, const float *w, int transposed, void *image, float *inv_scale,
                                      rtk_stream_t stream);
RTK_EXPORT int rtk_cost_volume_split16_shared(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                              const int64_t *knn_idx, const float *p1, const float *p2, const float *wd_packed,
                                              const void *split_images16, const float *image_scales, const float *bias2,
                                              const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch, int workgroups,
                                              rtk_stream_t stream);
RTK_EXPORT int rtk_cost_volume_split16_term(int samples, int n1, int n2, const float *xyz1, const float *xyz2,
                                            const int64_t *knn_idx, const float *p1, const float *p2, const float *sample_term,
                                            const float *wd_packed, const void *split_images16, const float *image_scales,
                                            const float *bias2, const float *bias3, const rtk_layer_t *wn, float *out, int out_pitch,
                                            int workgroups, rtk_stream_t stream);
/* rtk_sa_scale for the scales whose MLP is offset layer (c1 = 32 or 64 channels) + ONE layer c1 -> 64, nsample 16 or 32 (sa2 scale 1,
 * sa3 scales 0 and 1 of the PNHead): same arguments, the layer as its split image + inverse scale (rtk_pack_split_layer(64, c1, ...)) + fp32 bias.
 * (A sample whose q rows span 2^32 bytes or more, n * q_pitch * 4, is computed by the serial loop: same bits.) */
RTK_EXPORT int rtk_sa_scale_split(int samples, int n, int npoint, int nsample, const float *xyz, const float *new_xyz,
                                  const int *idx, const float *q, int q_pitch, int c1, const float *w1xyz_packed,
                                  const void *split_image, const float *image_scale, const float *bias2, float *out, int out_pitch,
                                  int out_offset, const int *src_nuniq, const int *dst_nuniq, rtk_stream_t stream);
/* ... with the serial tile loop: see rtk_sa_scale_serial.  Same arguments, bit-identical result. */
RTK_EXPORT int rtk_sa_scale_split_serial(int samples, int n, int npoint, int nsample, const float *xyz, const float *new_xyz,
                                         const int *idx, const float *q, int q_pitch, int c1, const float *w1xyz_packed,
                                         const void *split_image, const float *image_scale, const float *bias2, float *out,
                                         int out_pitch, int out_offset, const int *src_nuniq, const int *dst_nuniq,
                                         rtk_stream_t stream);
RTK_EXPORT int rtk_split_mlp2(int positions, const float *x, const void *images, const float *image_scales, const float *bias1,
                              const float *bias2, float *y, rtk_stream_t stream);

/* Layout glue of Track4D.backbone (models/track4d.py:104-105): (B,3,N)/(B,2,N) channel-major inputs of both
 * frames -> xyz (2B,N,3) and raw (2B,N,4) = (RCS, v_r, 0, 0) point-major, frame 1 first. */
RTK_EXPORT int rtk_prepare_inputs(int b, int n, const float *pc1, const float *pc2, const float *feature1,
                                  const float *feature2, float *xyz, float *raw, rtk_stream_t stream);

/* furthest_point_sample + gather_operation of a set-abstraction level in one launch
 * (lib/pointnet2_modules.py:30-35): same selection rule as rtk_furthest_point_sampling with the
 * min-distance scratch held on chip (initialised to 1e10).  idx (B,npoint) int32, new_xyz (B,npoint,3);
 * nuniq (B) int32 (optional) = number of picks made before the cloud was exhausted (every later pick is
 * point 0, i.e. a duplicate of centroid 0).  tie (B) int32 (optional) = the LAST round in which more than one point attained a
 * non-zero maximum (the pick then depended on the reference's tie rule), 0 if there was none.
 * n_valid (B) int32 (optional): padded batch -- sample b's cloud is its first n_valid[b] <= n points (row pitch n); the
 * selection, INCLUDING the size-dependent tie rule (block = 2^floor(log2 n_valid[b])), is that of the unpadded cloud.
 * snap (B,n) fp32 + first_tie (B) int32 (optional, together): at the first round with a tie, that round's number and the
 * min-distance state it started from (by point index) -- what rtk_fps_relevel needs to resume there.  Rows without a tie are not
 * written. */
RTK_EXPORT int rtk_fps_centroids(int b, int n, int npoint, const float *xyz, int *idx, float *new_xyz, int *nuniq,
                                 int *tie, const int *n_valid, float *snap, int *first_tie, rtk_stream_t stream);

/* rtk_knn_point over padded batches: only points[b][0 .. n_valid[b]) are candidates (n_valid (B) int32; n_valid[b] >= n: all n rows).
 * A sample with FEWER valid points than neighbours asked for, n_valid[b] < k, takes rows [0, k) as its candidates: the caller's padding
 * rows n_valid[b] .. k-1 take part with the coordinates they hold (copies of row 0 under vod_gt.pad_frame_pairs: they tie with row 0
 * and follow it in index order), so the k indices written are always distinct rows below max(n_valid[b], k).  n_valid == NULL:
 * rtk_knn_point. */
RTK_EXPORT int rtk_knn_point_masked(int b, int s, int n, int k, const float *query, const float *points, int64_t *idx,
                                    const int *n_valid, rtk_stream_t stream);

/* Levels 2 .. 1+levels of a PNHead (model_utils.py:415-417): furthest point sampling of npoint out of the npoint
 * centroids of the previous level, starting from the level-1 centroids xyz1 (B,npoint,3) with their counters
 * nuniq1 / tie (B) from rtk_fps_centroids.  One launch per level; decided per cloud on the device: a cloud whose previous level
 * had no tie is the identity on the coordinates (proof at rtk_fps_relevel in csrc/ops_pointnet2.hip) and is only copied, a tied
 * cloud runs the selection of the level-1 kernel -- stopping as soon as, past the previous level's last tie, the picked set is a
 * prefix again (the rest is then the identity).  idx (levels,B,npoint) int32, new_xyz (levels,B,npoint,3), nuniq (levels,B);
 * tie_work (levels,B) int32: the levels' own tie counters (required for levels > 1).
 * idx1 (B,npoint) / snap1 (B,snap_pitch) / first_tie1 (B) from rtk_fps_centroids (optional, together; levels <= 2): tied clouds
 * resume at level 1's first tied round from the state saved there instead of at round 1. */
RTK_EXPORT int rtk_fps_relevel(int b, int npoint, int levels, const float *xyz1, const int *nuniq1, const int *tie,
                               int *idx, float *new_xyz, int *nuniq, int *tie_work, const int *idx1, const float *snap1,
                               int snap_pitch, const int *first_tie1, rtk_stream_t stream);

/* One time step of nn.GRU(hidden, hidden, layers) on a length-1 sequence (model_utils.py:279,296).
 * x (B,H); h_in, h_out (L,B,H); w_ih, w_hh TRANSPOSED (L,H,3H) = weight_{ih,hh}_l{l}.T, gate order (r,z,n);
 * b_ih, b_hh (L,3H); y (B,H) = h_out[L-1].  H <= 128. */
RTK_EXPORT int rtk_gru_step(int b, int layers, int hidden, const float *x, const float *h_in, const float *w_ih,
                            const float *w_hh, const float *b_ih, const float *b_hh, float *h_out, float *y,
                            rtk_stream_t stream);

/* rtk_gru_step with an epilogue: head_out (B, head_cout) = head_w y + head_bias, head_wt = head_w TRANSPOSED (H, head_cout) -- the
 * per-sample bias the flow head's first layer takes from the GRU output (model_utils.py:297-300).  H % 16 == 0. */
RTK_EXPORT int rtk_gru_step_head(int b, int layers, int hidden, const float *x, const float *h_in, const float *w_ih,
                                 const float *w_hh, const float *b_ih, const float *b_hh, float *h_out, float *y, const float *head_wt,
                                 const float *head_bias, float *head_out, int head_cout, rtk_stream_t stream);

/* Everything that is a function of a sample's global (max-pooled) feature g (samples, cin) in one launch (models/track4d.py:89-95
 * broadcasts it over the points and concatenates it to per-point inputs; a concatenated global half of a layer's input is a
 * per-sample bias of that layer): jobs[j]: out[(s - s0), :cout] = W g[s] + bias for s in [s0, s0 + count), wt = W TRANSPOSED
 * (cin, cout) fp32; and, with bcast, bcast[(s n + r) bcast_pitch + c] = g[s][c] for every row r < n of every sample.  cin % 32 == 0.
 * A job with wt2 (W2 transposed, (cin, cout)) is paired: out[(s - s0)] = (W g[s] + bias) + W2 g[s - s0 + s2], both maps evaluated
 * as two jobs of their own would be (the second without bias), then added with one rounding -- bit for bit the sum of those two
 * jobs' outputs.  wt2 = NULL: s2 is ignored. */
#define RTK_GT_MAX_JOBS 4
typedef struct {
    const float *wt, *bias;      /* (cin, cout), (cout) or NULL */
    float *out;                  /* (count, out_pitch) */
    int cout, s0, count, out_pitch;
    const float *wt2;            /* (cin, cout) or NULL */
    int s2;                      /* with wt2: s2 + count <= samples */
} rtk_gterm_job_t;
RTK_EXPORT int rtk_global_terms(int samples, int cin, const float *g, int njobs, const rtk_gterm_job_t *jobs, float *bcast, int bcast_pitch,
                                int n, rtk_stream_t stream);

/* Up to RTK_COPY_MAX_JOBS device-to-device copies in one launch (sizes in bytes, multiples of 4; pointers 4-byte aligned). */
#define RTK_COPY_MAX_JOBS 8
typedef struct {
    const void *src;
    void *dst;
    long bytes;
} rtk_copy_job_t;
RTK_EXPORT int rtk_copy_multi(int njobs, const rtk_copy_job_t *jobs, rtk_stream_t stream);

/* (rows = samples*n, pitch) point-major -> (samples, channels, n) channel-major at channel offset
 * dst_channel_offset of a (samples, dst_channels, n) tensor; per_sample != 0 broadcasts a (samples, pitch)
 * source over the n points (the global-feature halves of pc{1,2}_features, models/track4d.py:89-95). */
RTK_EXPORT int rtk_to_channel_major(int samples, int n, int channels, const float *src, int src_pitch, int per_sample,
                                    float *dst, int dst_channels, int dst_channel_offset, rtk_stream_t stream);

/* Both ball queries of one MSG level in a single scan of the source cloud (lib/pointnet2_modules.py:37-38 issues
 * one ball_query per scale over the same centroids): identical results to two rtk_ball_query calls with
 * (radius1, nsample1) and (radius2, nsample2), radius1 <= radius2.  idx1/idx2 zero-initialised by the caller.
 * nuniq (optional, (B)): centroids >= nuniq[b] (duplicates of centroid 0, see rtk_fps_centroids) are skipped -- their rows keep the
 * caller's zeros, except that the rows up to the next multiple of 32 are WRITTEN as zeros (round 6: a consumer's last tile may load
 * them before it masks them; rtk_geometry_tables relies on this instead of a zero-filled workspace).  An empty ball's row is written
 * as zeros as well (what the caller's initialisation leaves there in the reference). */
RTK_EXPORT int rtk_ball_query_pair(int b, int n, int npoint, float radius1, int nsample1, float radius2, int nsample2,
                                   const float *new_xyz, const float *xyz, int *idx1, int *idx2, const int *nuniq,
                                   rtk_stream_t stream);

/* rtk_three_nn restricted to the non-duplicate unknown rows (rows >= unknown_nuniq[b] are not computed) and aware of
 * duplicate known rows (known rows >= known_nuniq[b] are copies of known row 0: only the unique prefix is scanned,
 * the result is identical to the full scan).  Either counter may be NULL.
 * Rows are written in whole chunks of 64 queries: rows [unknown_nuniq[b], roundup(unknown_nuniq[b], 64)) below n are written too (valid
 * indices and distances, which no consumer may rely on); rows at or past roundup(unknown_nuniq[b], 64) keep the caller's bits. */
RTK_EXPORT int rtk_three_nn_masked(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                                   const int *unknown_nuniq, const int *known_nuniq, rtk_stream_t stream);

/* The geometry of a batch of frame pairs in two launches (round 6) -- bit for bit the tables of the eleven launches they replace
 * (sampling_gpu.cu:94-209 x 3 levels, ball_query_gpu.cu:9-45 x 6, interpolate_gpu.cu:81-124 x 3, model_utils.py:85-99 x 2).
 *
 * rtk_geometry_front: everything that depends on the input clouds only.  frame1 / frame2: the b clouds of each frame,
 * channel_major != 0: the API's (B,3,n) tensors, else point-major (B,n,3); clouds = 2 b, or b (frame 1 only, frame2 unused, no kNN; S below
 * stands for `clouds`).  With xyz / raw (together, with the (B,2,n) features):
 * rtk_prepare_inputs' outputs.  The three PNHead levels of rtk_fps_centroids + rtk_fps_relevel: fps_idx (3,S,npoint) int32,
 * new_xyz (3,S,npoint,3), nuniq (3,S), tie (3,S), first_tie (S) (zero-initialised), snap (S,n).  n_valid (S) optional.
 * knn12 / knn11 (B,n,16) int64 (optional, together): rtk_knn_point_masked of frame 1 in frame 2 / in frame 1, k = 16.
 * q1_w (q1_cout, 2) / q1_out (S n, q1_cout) (optional, together, with xyz / raw): q1_out = q1_w . (feature row) -- the encoder's first
 * per-point projection (lib/pointnet2_modules.py:37-53: layer 1 of sa1's MLPs restricted to the two feature channels), no bias.
 * n <= 2048, npoint <= 512. */
RTK_EXPORT int rtk_geometry_front(int b, int clouds, int n, int npoint, const float *frame1, const float *frame2, int channel_major,
                                  const float *feature1, const float *feature2, float *xyz, float *raw, int *fps_idx, float *new_xyz,
                                  int *nuniq, int *tie, int *first_tie, float *snap, const int *n_valid, int64_t *knn12, int64_t *knn11,
                                  const float *q1_w, float *q1_out, int q1_cout, rtk_stream_t stream);
/* rtk_geometry_tables: the six ball queries (rtk_ball_query_pair per level) and the three three-NN tables (rtk_three_nn_masked) of a
 * PNHead.  xyz0 (S,n,3) point-major clouds; new_xyz / nuniq as written by rtk_geometry_front.  radii, nsamples: HOST arrays of six
 * (level-major, scale 0 then 1, radii ascending within a level); ball: host array of six device tables (S,npoint,nsample) int32,
 * zero-initialised by the caller; nn_idx / nn_dist2: host arrays of three device tables [fp3, fp2, fp1]: (S,npoint,3) x 2, (S,n,3). */
RTK_EXPORT int rtk_geometry_tables(int samples, int n, int npoint, const float *xyz0, const float *new_xyz, const int *nuniq,
                                   const float *radii, const int *nsamples, int *const *ball, int *const *nn_idx, float *const *nn_dist2,
                                   rtk_stream_t stream);

/* Several rtk_to_channel_major jobs in one launch. */
typedef struct {
    const float *src; float *dst;
    int channels, src_pitch, per_sample, dst_channels, dst_channel_offset;
} rtk_layout_job_t;
RTK_EXPORT int rtk_to_channel_major_multi(int samples, int n, int njobs, const rtk_layout_job_t *jobs, rtk_stream_t stream);

/* Object association (models/track4d.py:166-180, models/utils/track4d_utils.py:405-434): log-space Sinkhorn normalisation
 * with a dustbin row and column, all `iters` iterations in one launch.  scores (m,n) fp32 (previous x current object
 * affinities), alpha the dustbin score; out (m+1, n+1) = log_optimal_transport(scores, alpha, iters).  One workgroup:
 * (m+1)(n+2) floats must fit 64 KiB of LDS (m, n up to ~120 objects). */
RTK_EXPORT int rtk_log_sinkhorn(int m, int n, const float *scores, float alpha, int iters, float *out, rtk_stream_t stream);

/* Moving-point clustering (models/track4d.py:108-126; sklearn.cluster.DBSCAN(eps, min_samples) in the reference, on the host).
 * feat: channel-major (C, pitch) per-point tensor of ONE frame; channels (8) int32 DEVICE array = the feature channels
 * entering the distance; score (n): a point takes part iff score > threshold (the motion-segmentation probability).
 * labels (n) int32: sklearn's cluster ids restricted to the participating points (numbered by first core point), -1 = noise or
 * not participating.  One workgroup; its tables live in LDS up to ~2900 points and in a stream-ordered global workspace beyond
 * (n <= 65536; all pairs are tested by that one workgroup). */
RTK_EXPORT int rtk_dbscan(int n, const float *feat, int pitch, const int *channels, const float *score, float threshold, double eps,
                          int min_samples, int *labels, rtk_stream_t stream);

/* ---- Batched tracking (ratrack_amd/tracker.py): B independent sequences, one launch per stage per frame -------------------------
 * Detection and association of the post-backbone half of Track4D.forward for every stream of a batch at once, without a host round
 * trip.  Per stream b: K = max_objects object slots; objects are numbered in the reference's order (by their first member point).
 * Descriptors are the 141-d vectors of association.object_descriptor:
 *   [centre(3) | var xyz(3) | max prop(128) | mean flow(3) | mean (RCS, v_r)(2) | var (RCS, v_r)(2)]. */
#define RTK_DESC 141

/* Element (b, c, p) of a (B, C, N) tensor at ptr[b * sb + c * sc + p * sp] (strides in floats): the backbone's outputs are
 * permuted views of point-major buffers and are read in place. */
typedef struct {
    const float *ptr;
    long long sb, sc, sp;
} rtk_bcn_view_t;

/* One frame of the batch: pc1 (B,3,N), flow (B,3,N), feature1 (B,2,N) = (RCS, v_r), prop (B,128,N), cls (B,1,N) (sc unused). */
typedef struct {
    int B, N;
    rtk_bcn_view_t pc1, flow, feature1, prop, cls;
    const int *n_valid;            /* (B) DEVICE: frame-1 point counts (row 0 of a padded batch's n_valid), or NULL: N points */
    const unsigned char *active;   /* (B) DEVICE: 0 = the stream sits this frame out, or NULL: every stream is active */
} rtk_track_frame_t;

/* rtk_dbscan_batched: mover selection (cls > threshold over the stream's n_valid columns) + DBSCAN on the channels
 * (xyz, flow, v_r, prop[0]), per stream, labels identical to rtk_dbscan.  Outputs: labels (B,N) cluster ids (-1: noise, non-mover,
 * padding or inactive), obj (B,N) object index in reference order (-1: none), num_objects (B) = min(objects, K), flags (B):
 * bit 0 = more than K objects (objects K.. are not reported), bit 1 = n_valid outside [0, N] (clamped).  Tables of a stream live
 * in LDS when they fit 128 KiB, else in its slice of `work` (B * N * RTK_DBSCAN_POINT_BYTES bytes; may be NULL when every table
 * fits).  One workgroup per stream. */
#define RTK_DBSCAN_POINT_BYTES 48
RTK_EXPORT int rtk_dbscan_batched(const rtk_track_frame_t *frame, float threshold, double eps, int min_samples, int K, int *labels,
                                  int *obj, int *num_objects, int *flags, void *work, long long work_bytes, rtk_stream_t stream);

/* rtk_object_descriptors: desc (B,K,141) of every object of every active stream (points in index order; two-pass population
 * variance, both sums compensated: as accurate for an object of 500 points 80 m away as for one of two points at the origin).
 * Inactive streams carry their previous descriptors over: desc[b][:prev_count[b]] = desc_prev[b][:prev_count[b]] bit for bit
 * (prev_count clamped to [0, K]).  Nothing else is written: rows >= num_objects[b] of an active stream and rows >= prev_count[b] of an
 * inactive one keep what the caller's buffer held (rtk_track_memory puts its survivors there; no reader looks past the counts).
 * Only the first n_valid[b] columns of obj are read; num_objects[b] <= K is the caller's (rtk_dbscan_batched's) guarantee. */
RTK_EXPORT int rtk_object_descriptors(const rtk_track_frame_t *frame, int K, const int *obj, const int *num_objects,
                                      const int *prev_count, const float *desc_prev, float *desc, rtk_stream_t stream);

/* rtk_affinity_pairs: the Affinity MLP 141 -> 564 -> 282 -> 70 -> 35 -> 1 (ReLU, then sigmoid) on desc[b][j] - desc_prev[b][i]
 * for the live pairs i < m_b (previous objects; 0 on a reset stream), j < num_objects[b] only: aff[b][i][j] (B,K,K).
 * weights: packed by RTK_AFFINITY_WEIGHTS floats = for each layer its transposed weight (Cin, Cout) then its bias (Cout). */
#define RTK_AFFINITY_WEIGHTS (141 * 564 + 564 + 564 * 282 + 282 + 282 * 70 + 70 + 70 * 35 + 35 + 35 + 1)
RTK_EXPORT int rtk_affinity_pairs(int B, int K, const float *weights, const float *desc_prev, const int *prev_count,
                                  const unsigned char *reset, const float *desc, const int *num_objects, float *aff,
                                  rtk_stream_t stream);

/* rtk_associate_batched: per stream, the log-Sinkhorn of rtk_log_sinkhorn (same arithmetic; `iters` iterations, dustbin `alpha`)
 * on its live (m_b, n_b) block of aff, the mutual-best assignment (exact ties: the LOWEST index wins), the track IDs
 * (fresh from counter[b] in current-object order when unmatched or aff < 0.01, else the previous object's ID with conf = aff) and
 * point_track_id (B,N).  Writes object_ids / object_conf / indices1 (B,K) (-1 / 0 / -1 past num_objects), num_prev (B) = m_b,
 * counter (B) in place, and the next state ids (B,K), count (B).  Inactive streams: ids = prev_ids, count = prev_count, no objects.
 * scores: NULL, or (B, K+1, K+1): each stream's whole (m_b+1, n_b+1) Sinkhorn output (rtk_log_sinkhorn's `out`, row stride K+1);
 * nothing outside that block is written, and nothing at all for a stream that is inactive, reset, or has m_b = 0 or n_b = 0 (no
 * plan is computed there).  aff is read inside the live (m_b, n_b) block only.  The threshold is the double 0.01 against the fp32
 * aff widened: float32(0.01) itself is below it and starts a fresh track, as in the reference.
 * One workgroup per stream; its LDS holds the (K+1) x (K+1) table (about 66 KiB at K = 128). */
RTK_EXPORT int rtk_associate_batched(int B, int N, int K, const unsigned char *active, const unsigned char *reset, const float *aff,
                                     const int *num_objects, const int *obj, const int *prev_ids, const int *prev_count, float alpha,
                                     int iters, int *counter, int *ids, int *count, int *object_ids, float *object_conf, int *indices1,
                                     int *num_prev, int *point_track_id, float *scores, rtk_stream_t stream);

/* rtk_associate_optimal: rtk_associate_batched with the decision replaced by an EXACT maximum-weight one-to-one assignment
 * (csrc/track_assign.hip, csrc/lds_assignment.h: la_solve_dense) -- issued INSTEAD of it, never with it; no Sinkhorn runs.  The live
 * sizes are rtk_associate_batched's: m_b = prev_count[b] clamped to [0, K], 0 on a reset stream; n_b = num_objects[b] clamped to [0, K].
 *   admissible  pair (i, j), i < m_b, j < n_b, is admissible iff (double)aff[b][i][j] >= min_affinity.  A NaN is not admissible.
 *               min_affinity lies in [0.01, 1]; outside that range, or a NaN, the call is refused.  0.01 is the reference's confidence
 *               threshold: as in rtk_associate_batched float32(0.01) itself is below the double 0.01 and is not admissible.
 *   weight      an admissible pair weighs (int)(aff * 268435456.0f) (2^28, truncated; the product is exact in fp32, so the weight is a
 *               function of the aff word alone): between 2 684 354 and 2^28 for an aff in [0.01, 1].  An aff above 1 (no sigmoid gives
 *               one) weighs as 1.  An inadmissible pair weighs 0 and is no edge.
 *   decision    previous rows are the rows and current objects the columns of one assignment problem per stream.  The matching
 *               takes every row and every column at most once, uses admissible pairs only, and has the largest total weight any such
 *               matching can have; that total is unique.  Where several matchings reach it the choice is a deterministic function of
 *               the weight block (rows enter in index order, ties go to the smaller column index); nothing more is promised about it.
 *   outputs     exactly rtk_associate_batched's.  Object j matched to row i: indices1 = i, object_ids = prev_ids[i], object_conf =
 *               the aff word of the pair (at least the gate, hence != 0: the "matched" rule of rtk_track_memory holds as written).
 *               An unmatched object: indices1 = -1, object_conf = 0, a fresh ID from counter[b] in current-object order.  Rows past
 *               n_b: -1 / 0 / -1.  num_prev = m_b, count = n_b, ids[j] = object_ids[j] for j < n_b (rows past n_b are not written),
 *               counter in place, point_track_id (B,N) = the ID of the point's object (obj in [0, n_b)) or -1.  With m_b = 0 or
 *               n_b = 0 no solve runs and every object is fresh.  Inactive streams: ids = prev_ids (all K rows), count = m_b before
 *               the reset rule (prev_count clamped), num_prev = 0, no objects, point_track_id = -1, counter untouched.
 *   total       NULL, or (B) long long: the matching's weight; 0 where no solve ran; untouched for an inactive stream.
 * aff is read inside the live (m_b, n_b) block only.  Plain stores only: two runs give the same bits.  One one-wave workgroup per
 * stream; its LDS holds the K x K weight block, the solver's tables (K + 5 K words) and the K new IDs: rtk_associate_optimal_lds_bytes(K),
 * 160 752 bytes at K = 197 = rtk_track_max_objects(). */
RTK_EXPORT int rtk_associate_optimal(int B, int N, int K, const unsigned char *active, const unsigned char *reset, const float *aff,
                                     const int *num_objects, const int *obj, const int *prev_ids, const int *prev_count,
                                     double min_affinity, int *counter, int *ids, int *count, int *object_ids, float *object_conf,
                                     int *indices1, int *num_prev, int *point_track_id, long long *total, rtk_stream_t stream);
/* The dynamic LDS of one workgroup of rtk_associate_optimal at K object slots, in bytes (a host function); -1 for a K below 1. */
RTK_EXPORT int rtk_associate_optimal_lds_bytes(int K);

/* rtk_track_memory: track memory (a lost track coasts for up to max_age frames) -- the state advance of a tracker that keeps lost
 * tracks, issued after rtk_associate_batched on the same stream.  The table of a stream (ids, desc, age, hits, its row count `count`,
 * and n_det = how many of its leading rows are the last active frame's detections; the rows after them are coasted tracks) is
 * double-buffered: prev_* is read, the others are written.  rtk_object_descriptors and rtk_associate_batched have already written
 * desc / ids of the current rows j < n_b = num_objects[b]; m_b is the number of previous rows (prev_count[b]; 0 on a reset stream).
 *   matched    previous row i < m_b is matched iff some j < n_b has indices1[b][j] == i and object_conf[b][j] != 0 (object j
 *              inherited that row's ID; mutual-best gives at most one such j).
 *   current    rows j < n_b: age = 0, hits = prev_hits[i] + 1 when inherited from row i, else 1; n_det = n_b.
 *   survivors  the previous rows i < m_b that are not matched and have prev_age[i] + 1 <= max_age, in increasing i: the s-th becomes
 *              row n_b + s when n_b + s < K -- ids and the 141 descriptor floats copied bit for bit (no motion model: a coasted
 *              track holds its last descriptor), age = prev_age[i] + 1, hits = prev_hits[i].
 *   count      min(K, n_b + S), S the number of survivors.  Survivors that do not fit are dropped, the last in table order first,
 *              and bit 2 (value 4) of flags[b] is set.  Rows past count: ids = -1, age = 0, hits = 0.
 *   reset      the previous table is ignored: no survivors, every current row has hits = 1.
 *   inactive   ids, age, hits, n_det, count equal the previous table's (ids and count by rtk_associate_batched, the descriptors by
 *              rtk_object_descriptors): a track does not age while its stream sits a frame out.
 *   An active frame with n_b = 0 ages every previous row.
 * Per-step outputs: object_hits (B,K) = hits of current object j (0 past n_b); object_gap (B,K) = prev_age of the row object j
 * inherited from (0: seen last frame, g: re-acquired after g missed frames; -1: fresh ID or past n_b); num_coasted (B) = count - n_det
 * of the new table (= count - n_b on an active stream).
 * active / reset may be NULL (all active / none reset).  One workgroup per stream, plain stores only: every run gives the same bits.
 * (Coasted tracks that move with their track's velocity: rtk_track_memory_motion below, a separate entry point.) */
RTK_EXPORT int rtk_track_memory(int B, int K, int max_age, const unsigned char *active, const unsigned char *reset,
                                const int *num_objects, const int *indices1, const float *object_conf, const int *prev_ids,
                                const int *prev_age, const int *prev_hits, const int *prev_n_det, const int *prev_count,
                                const float *desc_prev, int *ids, int *age, int *hits, int *n_det, int *count, float *desc, int *flags,
                                int *object_hits, int *object_gap, int *num_coasted, rtk_stream_t stream);

/* rtk_track_memory_motion: rtk_track_memory with a constant-velocity motion model (csrc/track_motion.hip) -- issued INSTEAD of it,
 * never with it.  Every row of the table carries a velocity, vel (B,K,3) fp32, double-buffered like the table (prev_vel is read,
 * vel is written; they must not alias): the object's displacement per frame in the sensor frame, taken from channels 134..136 of its
 * descriptor (its mean predicted scene flow, which includes the ego motion -- no pose is needed).  Everything stated for
 * rtk_track_memory holds unchanged: ids, age, hits, n_det, count, flags bit 2, object_hits, object_gap, num_coasted, and what a
 * reset, an inactive stream and an empty frame do.  In addition (`from` = the previous row current row j inherited its ID from, -1
 * when it did not; all arithmetic is fp32, every operation rounded on its own, no FMA):
 *   current    rows j < n_b, with f = desc[b][j][134..136] (written by rtk_object_descriptors; desc is read AND written here):
 *              vel[j] = f bit for bit when from < 0 or beta == 1, else vel[j] = v + beta * (f - v) with v = prev_vel[from] (a
 *              subtraction, a multiplication, an addition).  object_velocity[j] = vel[j].  The descriptor row is not touched.
 *   survivors  previous row i that becomes row r: the 141 descriptor words are copied bit for bit except channels 0..2, the centre:
 *              desc[r][c] = desc_prev[i][c] + prev_vel[i][c] (one addition), so a track that coasts g frames has moved g times;
 *              channels 134..136 keep the last measured flow.  vel[r] = prev_vel[i] bit for bit.
 *   reset      no survivors; every current row takes vel = f.
 *   inactive   vel = prev_vel for all K rows and no centre moves (no frame passed; rtk_object_descriptors carried the descriptors
 *              over); object_velocity = 0.
 *   Rows past count: vel = 0.  object_velocity past n_b: 0.
 * beta in (0, 1] (a NaN is refused): 1 = the velocity is the last measured mean flow, smaller = exponential smoothing along the
 * track.  One workgroup per stream, plain stores only: every run gives the same bits. */
RTK_EXPORT int rtk_track_memory_motion(int B, int K, int max_age, float beta, const unsigned char *active, const unsigned char *reset,
                                       const int *num_objects, const int *indices1, const float *object_conf, const int *prev_ids,
                                       const int *prev_age, const int *prev_hits, const int *prev_n_det, const int *prev_count,
                                       const float *desc_prev, const float *prev_vel, int *ids, int *age, int *hits, int *n_det,
                                       int *count, float *desc, float *vel, int *flags, int *object_hits, int *object_gap,
                                       int *num_coasted, float *object_velocity, rtk_stream_t stream);

/* The largest K (max_objects) the batched association accepts: its per-stream table must fit one workgroup's LDS. */
RTK_EXPORT int rtk_track_max_objects(void);

/* ---- The result log (csrc/track_results.hip, ratrack_amd/result_log.py): a tracked step's result file kept on the device ---------
 * A result file holds, per object of a frame in association order, its confidence, its track id and the xyz of its points in column
 * order (BatchedTracker.write_results).  The log keeps exactly that per stream, packed, with per-frame offsets and cursors that live on
 * the device, so that a step appends without a host round trip (a captured append replays correctly) and everything is downloaded once.
 * F frames, R records and P points per stream bound the memory.  Zero-initialised by the caller; only rtk_result_log_append writes it. */
#define RTK_RESULT_MAX_OBJECTS 256   /* object slots of a frame: RTK_SCORE_MAX_OBJECTS, the frame word's 16-bit count and the scan's width */
#define RTK_RESULT_FLAG_OBJECTS 1    /* a num_objects outside [0, K]: the frame was not logged */
#define RTK_RESULT_FLAG_STEP 2       /* the step's flags word had bit 0 or bit 1 set (object overflow, bad n_valid): not logged */
#define RTK_RESULT_FLAG_FULL 4       /* the frame needed more than what is left of F, R or P: not logged at all */
#define RTK_RESULT_FLAG_TRACKS 8     /* rtk_result_log_select: more track ids in one clip than the track table holds (2048) */

typedef struct {
    int F, R, P;
    int *cursor;                  /* (B,4) frames | records | points logged so far | unused (never written) */
    int *frame;                   /* (B,F,4) first record | first point | P_f + 65536 * (the frame began a clip) | 0: rtk_score_log_t's word */
    int *tag;                     /* (B,F,4) seq | index | points of the frame | the step's flags word */
    int *rec_track;               /* (B,R) per object, in order: its track id */
    float *rec_conf;              /* (B,R) its object_conf */
    int *rec_hits;                /* (B,R) its object_hits, 0 when the step has none */
    int *rec_size;                /* (B,R) its point count */
    float *points;                /* (B,P,3) xyz, object after object, inside an object in increasing column */
    int *flags;                   /* (B) sticky: RTK_RESULT_FLAG_OBJECTS | _STEP | _FULL */
} rtk_result_log_t;

/* rtk_result_log_append: one workgroup per stream.  pc1 (B,3,N) read in place, obj (B,N), num_objects (B), object_ids / object_conf
 * (B,K); object_hits (B,K), step_flags (B), reset (B), active (B) may be NULL (hits 0 / flags 0 / no clip mark / every stream active);
 * seq, index (B) int32 DEVICE words read at launch time.  Per active stream b with P_f = num_objects[b]:
 *   refusals   P_f outside [0, K]: RTK_RESULT_FLAG_OBJECTS; step_flags[b] & 3: RTK_RESULT_FLAG_STEP (both where both hold); else a
 *              frame that needs a frame slot, P_f records or its points beyond F / R / P: RTK_RESULT_FLAG_FULL.  A refused frame
 *              writes nothing but the flag and moves no cursor.
 *   records    record j < P_f = (object_ids[j], object_conf[j], object_hits[j] or 0, size_j), size_j the columns p with obj[b][p] == j.
 *   points     the xyz of those columns, object after object in j order, inside an object in increasing p (a STABLE grouping; columns
 *              with obj outside [0, P_f) belong to nothing; an object may be empty).
 *   frame      (first record, first point, P_f + 65536 * (reset[b] != 0), 0), tag (seq[b], index[b], points, step_flags[b] or 0);
 *              the three cursors advance.  An inactive stream changes no word.
 * Every word has one writer and plain stores: the same bits on every run; nothing at or beyond the new cursors is touched.  Static LDS:
 * a counter per (wave, object slot), 4 KiB.  K <= RTK_RESULT_MAX_OBJECTS; B * N, B * 4 F, B * R and B * 3 P below 2^31. */
RTK_EXPORT int rtk_result_log_append(int B, int N, int K, const rtk_bcn_view_t *pc1, const int *obj, const int *num_objects,
                                     const int *object_ids, const float *object_conf, const int *object_hits, const int *step_flags,
                                     const int *seq, const int *index, const unsigned char *reset, const unsigned char *active,
                                     const rtk_result_log_t *log, rtk_stream_t stream);

/* rtk_result_log_select: which records a result file keeps.  One workgroup per stream; reads the log, writes its four outputs.
 *   clip       a maximal run of the stream's logged frames in which only the first may carry the clip mark.
 *   track      a (stream, clip, track id); n_t its records in the clip; its score the float64 sum of their fp32 rec_conf in log order
 *              divided by (double)n_t: rtk_score_track_means' score (rtk_score.h, "the confidence sweep"), the same bits.
 *   keep       1 iff !(score < tau) && (min_hits <= 1 || rec_hits >= min_hits) && n_t >= min_track_frames; tau = *threshold when
 *              threshold (a DEVICE scalar) is not NULL, else threshold_value (-infinity keeps every score).  min_hits = 1 asks nothing,
 *              as in BatchedTracker.write_results: a frame logged without hit counts holds rec_hits = 0 and is not emptied by it.
 * keep (B,R) uint8, track_score (B,R) float64, track_frames (B,R) int32 are written for the records below the stream's cursor only.
 * flags (B) is WRITTEN: 0, or RTK_RESULT_FLAG_TRACKS for a stream with a clip of more track ids than the table holds (2048, a clip
 * within a wave's width of that may be refused too); the outputs of that clip and of the stream's later clips are then not written.
 * The log is walked with the scorer's clamps (csrc/score_log_walk.h), so a foreign buffer is never read out of bounds. */
RTK_EXPORT int rtk_result_log_select(int B, const rtk_result_log_t *log, const double *threshold, double threshold_value, int min_hits,
                                     int min_track_frames, unsigned char *keep, double *track_score, int *track_frames, int *flags,
                                     rtk_stream_t stream);

/* ---- Oriented boxes (csrc/track_boxes.hip, csrc/box_fit.h, ratrack_amd/boxes.py): position, size and heading of a tracked object -----
 * The box of an object is the minimum-area rectangle around its points in the bird's-eye view (x, y), with the points' z range for
 * its height.  THE FITTING RULE.  An object is its n points in the order the result log keeps them (increasing column); coordinates
 * are the fp32 values widened to float64, all arithmetic is float64, and every product, sum, quotient and square root is rounded on
 * its own (no FMA).
 *   extremes    min and max pick one of the values; an extreme that is a zero of either sign is taken as +0 (x + 0.0), so that no
 *               order of comparisons shows in a bit.
 *   empty       n == 0: the eight box words are 0, valid = 0, cand = -1.  Any coordinate (x, y or z) that is not finite: the eight
 *               words are 0, valid = -1, cand = -1.
 *   height      cz = (zmin + zmax) / 2, h = max(zmax - zmin, min_extent).
 *   candidates  directions d = (d_x, d_y).  Candidate 0 is (1, 0).  Candidate c = 1 + rank(i, j) belongs to the pair i < j, the pairs
 *               in lexicographic order (rank(i, j) = i (2 n - i - 1) / 2 + j - i - 1), with d = (x_j - x_i, y_j - y_i).  A pair with
 *               q = d_x d_x + d_y d_y == 0 is skipped and keeps its index.  The pairs are a superset of the hull's edges, so the
 *               smallest area among them is that of the minimum-area enclosing rectangle.
 *   area        s_k = d_x x_k + d_y y_k, t_k = d_x y_k - d_y x_k; S = max s - min s, T = max t - min t; area = (S T) / q.  Nothing
 *               is normalised before the comparison: for small-integer inputs every term is exact.
 *   winner      the smallest area; among equal areas the smallest c.  A function of the points alone, not of how the work is split.
 *   box         r = sqrt(q), len_s = S / r, len_t = T / r; ms = (smin + smax) / 2, mt = (tmin + tmax) / 2;
 *               cx = (ms d_x - mt d_y) / q, cy = (ms d_y + mt d_x) / q; yaw = atan2(d_y, d_x).  If len_t > len_s the two lengths are
 *               swapped and yaw = yaw + PI / 2 (the box has no front).  Then while yaw >= PI / 2: yaw = yaw - PI, and while
 *               yaw < -PI / 2: yaw = yaw + PI (PI the float64 nearest pi): yaw lies in [-pi/2, pi/2).
 *               l = max(the longer, min_extent), w = max(the shorter, min_extent).
 *   output      box = (cx, cy, cz, l, w, h, yaw, area), eight float64 words, area the winner's before any padding; cand (int32) the
 *               winner; valid (int32) n, 0 for an empty object, -1 for one with a coordinate that is not finite.
 *   cap         an object of more than RTK_BOX_MAX_POINTS points is fitted with candidate 0 alone -- the axis-aligned box, cand = 0
 *               -- and RTK_BOX_FLAG_AXIS is set in its stream's flags word.  A record costs at most 8 128 candidates x 128 points.
 * min_extent is a finite number >= 0 (else the call is refused).  Except for yaw (atan2 is not correctly rounded) every word is a
 * correctly rounded function of the points. */
#define RTK_BOX_MAX_POINTS 128       /* points of an object the candidate search takes: 2 KiB of (x, y) per wave */
#define RTK_BOX_FLAG_AXIS 1          /* an object above RTK_BOX_MAX_POINTS was fitted axis-aligned */
#define RTK_BOX_FLAG_OBJECTS 2       /* rtk_object_boxes: a num_objects outside [0, K]: nothing of the stream was fitted */

/* rtk_result_log_boxes: the box of every record below each stream's cursors.  One workgroup of four waves per stream; a wave takes
 * frames in turn and, inside a frame, record after record.  keep: NULL, or (B,R) uint8 (rtk_result_log_select's): only the records it
 * marks are fitted, the others are written as empty (eight zeros, cand = -1, valid = 0).  box (B,R,8) float64, cand (B,R) int32,
 * valid (B,R) int32 are written for the records below the stream's cursor only; nothing at or beyond it is touched.  flags (B) is
 * WRITTEN: 0 or RTK_BOX_FLAG_AXIS -- one record above the cap raises it for its stream.  The log is walked with the scorer's clamps
 * (csrc/score_log_walk.h) and every size is clamped to the points logged, so a foreign buffer is never read out of bounds.  No
 * allocation, no synchronisation; every word has one writer and plain stores: the same bits on every run.  Static LDS: 8 KiB. */
RTK_EXPORT int rtk_result_log_boxes(int B, const rtk_result_log_t *log, const unsigned char *keep, double min_extent, double *box,
                                    int *cand, int *valid, int *flags, rtk_stream_t stream);

/* rtk_object_boxes: the same for a live step.  pc1 (B,3,N) read in place, obj (B,N), num_objects (B); object j < num_objects[b] is
 * the columns p with obj[b][p] == j in increasing p (rtk_result_log_append's grouping: what the log would hold for the step, so the
 * two entry points give a step's objects the same bits).  box (B,K,8), cand (B,K), valid (B,K): all K rows of every stream are
 * written, rows j >= num_objects[b] and every row of an inactive stream (active (B) uint8, may be NULL) as empty.  A num_objects
 * outside [0, K] is refused as rtk_result_log_append refuses it: RTK_BOX_FLAG_OBJECTS and K empty rows.  flags (B) is WRITTEN.
 * K <= RTK_RESULT_MAX_OBJECTS, B * N below 2^31.  One workgroup of four waves per stream; a wave takes objects in turn and scans the
 * stream's N columns for each.  No allocation, no synchronisation, one writer per word. */
RTK_EXPORT int rtk_object_boxes(int B, int N, int K, const rtk_bcn_view_t *pc1, const int *obj, const int *num_objects,
                                const unsigned char *active, double min_extent, double *box, int *cand, int *valid, int *flags,
                                rtk_stream_t stream);

/* ---- Filtered boxes (csrc/track_box_filter.hip, csrc/box_filter.h, ratrack_amd/boxes.py): the boxes of a track, not of a frame -----------
 * rtk_result_log_boxes gives every record the rectangle of that one frame's points.  This launch, run when the clip is over, links the
 * records of every track and runs a constant-velocity Kalman filter over (x, y, z, yaw, l, w, h, vx, vy, vz) along each track, with
 * an orientation correction before each update, optionally a backward (Rauch-Tung-Striebel) pass, and optionally a size taken from the
 * whole track.  F, H, Q, R and P0 of that ten-state filter couple a coordinate with nothing but its own velocity, so it is computed as
 * three two-state filters (x, y, z with their velocities) that share one covariance (P00, P01, P11) and four scalar filters: yaw with
 * Pyaw, and l, w, h that share Psize.  With r_* = 1, q_pos = q_yaw = q_size, symmetry = 2 and no gaps this IS the dense ten-state
 * filter (tests/test_box_filter_cpu.py holds the two together).
 * THE RULE.  All arithmetic is float64; every sum, product and quotient is rounded on its own (no FMA); nothing is transcendental and
 * every floor is exact, so every output word is a correctly rounded chain.  PI is the float64 nearest pi.
 *   clips       those of rtk_result_log_select, walked the same way; a track is a (stream, clip, track id).
 *   members     a record is ELIGIBLE if its input valid > 0, keep (where given) marks it and its id is not INT_MIN.  Of a frame's
 *               eligible records with one track id the one with the smallest index is the track's MEMBER in that frame; the others are
 *               not members and raise RTK_BOX_FLAG_DUPLICATE for their stream.  A member's frame number n is its frame's tag.index.
 *   non-members come out empty: box, vel, state, aligned all zero, valid 0, the four link words -1.
 *   segments    a track's members in log order.  The first starts a segment; a member whose k = n - n_prev (to the track's previous
 *               member) is below 1 or above max_gap starts a new one.  Links never leave a segment.
 *   measurement a member's input box read as z = (x, y, z, yaw, l, w, h).
 *   start       (first member of a segment) mean = (z, 0, 0, 0); P00 = p0, P01 = 0, P11 = p0_vel; Pyaw = Psize = p0; the aligned reading
 *               is the measurement as it is.
 *   predict     k times: per coordinate c of x, y, z: m_c = m_c + v_c.  a = P00 + P01; b = P01 + P11; P00 = (a + b) + q_pos; P01 = b;
 *               P11 = P11 + q_vel; Pyaw = Pyaw + q_yaw; Psize = Psize + q_size.
 *   align       H = (2 PI) / symmetry; d = yaw_z - yaw; t = floor(d / H + 0.5); yaw_z' = yaw + (d - t H).  With symmetry = 4 and t
 *               odd (t - 2 floor(t / 2) == 1) l_z and w_z are swapped.  symmetry 2: a rectangle without a front (a half turn changes
 *               nothing); 4: without a front and without a labelled side (a quarter turn swaps l and w; what fitted boxes are).  yaw is
 *               never wrapped inside the filter.
 *   update      S = P00 + r_pos; K0 = P00 / S; K1 = P01 / S; per coordinate y = z_c - m_c; m_c = m_c + K0 y; v_c = v_c + K1 y.
 *               P11 = P11 - K1 P01 (the old P01), then P01 = (1 - K0) P01, then P00 = (1 - K0) P00.
 *               Ky = Pyaw / (Pyaw + r_yaw); yaw = yaw + Ky (yaw_z' - yaw); Pyaw = (1 - Ky) Pyaw.
 *               Ks = Psize / (Psize + r_size); l, w, h each: m = m + Ks (z' - m), against the aligned reading; Psize = (1 - Ks) Psize.
 *   smooth      (smooth = 1) inside a segment from its last member backwards; the last member's smoothed mean is its filtered one.
 *               For member p whose successor lies k frames on: (m-, P-) = p's filtered state predicted k times;
 *               C00 = P00 + k P01; C01 = P01; C10 = P01 + k P11; C11 = P11 (p's filtered P); det = P-00 P-11 - P-01 P-01;
 *               G00 = (C00 P-11 - C01 P-01) / det; G01 = (C01 P-00 - C00 P-01) / det;
 *               G10 = (C10 P-11 - C11 P-01) / det; G11 = (C11 P-00 - C10 P-01) / det;
 *               per coordinate, e0 = the successor's smoothed m_c - m-_c, e1 = its smoothed v_c - v_c:
 *               m_c = m_c + (G00 e0 + G01 e1); v_c = v_c + (G10 e0 + G11 e1).
 *               yaw = yaw + (Pyaw / P-yaw) (yaw_successor - yaw); l, w, h likewise with Psize / P-size.  No smoothed covariance.
 *   extent      (size_rule = 1) for each of l, w, h: of the segment's n aligned readings, ordered by (value, record index), the one
 *               of 0-based rank (size_percent (n - 1)) / 100 (integer division) replaces that word of every member's final mean -- one
 *               of the measured values.  A track of partial views reaches the object's size this way; a percentile below 100 guards
 *               against a frame in which two clusters merged.  It looks at the whole segment: with smooth = 0 the result is then NOT
 *               causal either.
 *   output      from the final mean (smoothed if smooth, with the extent's sizes if size_rule): if w > l they are swapped and
 *               yaw = yaw + PI / 2; yaw = yaw - floor((yaw + PI / 2) / PI) PI, then one corrective -PI (yaw >= PI / 2) or +PI
 *               (yaw < -PI / 2).  out_box = (x, y, z, l, w, h, yaw, l w): rtk_result_log_boxes' layout.
 *               vel = (vx, vy, vz, the final mean's yaw before any of that: unwrapped).
 *               state = the FILTERED mean (x, y, z, yaw, l, w, h, vx, vy, vz), P00, P01, P11, Pyaw, Psize, 0.
 *               aligned = (yaw_z', l', w', h').   out_valid = the input's valid.
 *               link = previous member | gap k | next member | the segment's first member: record indices of the stream, -1 where
 *               there is none (a segment's first member has no previous member and no gap).
 * With smooth = 0 and size_rule = 0 a record's outputs depend on its track's earlier records only: the bits an in-step filter would
 * produce.  The filter runs in each frame's own sensor frame (no ego-motion compensation). */
#define RTK_BOX_FILTER_MAX_GAP 64    /* the largest max_gap: frames a segment may skip between two members */
#define RTK_BOX_FLAG_DUPLICATE 4     /* rtk_result_log_filter_boxes: a track id twice among a frame's eligible records */
#define RTK_BOX_FLAG_TRACKS 8        /* rtk_result_log_filter_boxes: more track ids in one clip than the track table holds (2048) */

typedef struct {
    double r_pos, r_yaw, r_size;            /* measurement variances: finite, > 0 */
    double q_pos, q_vel, q_yaw, q_size;     /* process variances per frame: finite, >= 0 */
    double p0, p0_vel;                      /* the initial variances: finite, > 0 */
    int symmetry;                           /* 2 or 4 */
    int max_gap;                            /* 1 ... RTK_BOX_FILTER_MAX_GAP */
    int smooth;                             /* 0 or 1 */
    int size_rule;                          /* 0: the filter's sizes, 1: the extent rule */
    int size_percent;                       /* 0 ... 100 */
} rtk_box_filter_t;

/* rtk_result_log_filter_boxes: the rule above over every stream's log.  One workgroup per stream.  keep: NULL or (B,R) uint8.
 * box (B,R,8) float64 and valid (B,R) int32 are rtk_result_log_boxes' outputs (or boxes from anywhere in that layout) and are only
 * read; the outputs must not alias them.  out_box (B,R,8), vel (B,R,4), state (B,R,16), aligned (B,R,4) float64, out_valid (B,R)
 * and link (B,R,4) int32 are written for the records below the stream's cursor only; nothing at or beyond it is touched.  flags (B) is
 * WRITTEN: 0, RTK_BOX_FLAG_DUPLICATE, or RTK_BOX_FLAG_TRACKS for a stream with a clip of more track ids than the table holds (as
 * rtk_result_log_select counts them, over all the clip's records): that clip and the stream's later clips come out empty, record for
 * record -- a clip is never filtered wrongly.  Parameters outside the ranges above refuse the call.  No allocation, no
 * synchronisation, one writer per word and plain stores: the same bits on every run, and the launch can be captured.  The log is
 * walked with the scorer's clamps and every link read back is checked against the cursor.  Static LDS: 48 KiB. */
RTK_EXPORT int rtk_result_log_filter_boxes(int B, const rtk_result_log_t *log, const unsigned char *keep, const double *box, const int *valid,
                                           const rtk_box_filter_t *par, double *out_box, int *out_valid, double *vel, double *state,
                                           double *aligned, int *link, int *flags, rtk_stream_t stream);

/* ---- Filtered boxes inside the step (csrc/track_box_step.hip, csrc/box_filter.h, ratrack_amd/boxes.py) ------------------------------------
 * The filter above, a frame at a time: the state of every track travels with the tracker's table, one launch per step after the
 * association and the box fit advances it IN PLACE and hands out, for every row of the table, the track's box and velocity now.
 * smooth and size_rule must be 0 (neither is causal); with them 0 a measured row gets the bits rtk_result_log_filter_boxes gives the
 * record the step would log, when every stream's frame index advances by one per active step.
 *   state (B,K,16) float64   a row has the layout of the offline launch's state: mean (x, y, z, yaw, l, w, h, vx, vy, vz), P00, P01, P11,
 *                            Pyaw, Psize, 0.
 *   since (B,K) int32        -1: the row has no filter; 0: the filter took a measurement this frame; s > 0: frames since its last one.
 * THE RULE, per stream b.  All arithmetic is box_filter.h's, called in the order given: float64, every operation rounded on its own.
 *   counts      count_prev, count_new and num_objects (n_b) are clamped to [0, K].
 *   inactive    (active[b] == 0) state and since keep every bit; all K output rows are empty: zeros, out_valid 0, gap -1.
 *   reset       (reset[b] and active[b]) the previous table is ignored: no row below has a previous row.
 *   previous    the previous row of new-table row r < count_new is the smallest i < count_prev with ids_prev[i] == ids_new[r]; an
 *               id < 0 matches nothing.  Ids are unique within a table, so this is a lookup; nothing of rtk_track_memory is needed.
 *   measured    r < min(n_b, count_new) and valid[b][r] > 0.  The reading is z = (box[0], box[1], box[2], box[6], box[3], box[4], box[5]).
 *               It CONTINUES if it has a previous row with since_prev >= 0 and k = since_prev + 1 <= max_gap: that state is loaded,
 *               predict k times, align, update; gap = k.  Otherwise it STARTS: start, the aligned reading is the measurement as it is,
 *               gap = -1.  Either way since = 0, out_valid = valid[b][r], aligned = (yaw_z', l', w', h').
 *   carried     r < count_new, not measured, a previous row with since_prev >= 0 (a coasted survivor; a detection without a valid
 *               box): the state is copied bit for bit, since = min(since_prev + 1, RTK_BOX_FILTER_MAX_GAP) (saturated, such a row can
 *               only start again), out_valid = 0, gap = -1, aligned = zeros.
 *   no filter   every other row below count_new and every row at or past it: state zeros, since = -1, the outputs empty.
 *   outputs     for a row with since >= 0, (out_box, vel) = output of a COPY of the state's mean after `since` position predictions
 *               (m_c = m_c + v_c, since times): a measured row's filtered box, a carried row's predicted one.  The stored state is never
 *               predicted eagerly, so the bits of a later update are those of the offline chain.
 * par outside the ranges above, smooth != 0, size_rule != 0 or K > RTK_RESULT_MAX_OBJECTS refuses the call.  active and reset may be NULL
 * (all active, none reset).  box (B,K,8) and valid (B,K) are rtk_object_boxes' outputs, or boxes from anywhere; the outputs must not
 * alias them.  out_box (B,K,8), out_valid (B,K), vel (B,K,4), aligned (B,K,4), gap (B,K): all K rows of every stream are written.
 * One workgroup of 256 lanes per stream, a lane per row; a lane reads its previous row's 16 words before a barrier and stores after
 * it.  No allocation, no synchronisation, one writer per word and plain stores: the same bits on every run, and the launch can be
 * captured.  Static LDS: 1 KiB. */
RTK_EXPORT int rtk_track_box_filter_step(int B, int K, const unsigned char *active, const unsigned char *reset, const int *ids_prev,
                                         const int *count_prev, const int *ids_new, const int *count_new, const int *num_objects,
                                         const double *box, const int *valid, const rtk_box_filter_t *par, double *state, int *since,
                                         double *out_box, int *out_valid, double *vel, double *aligned, int *gap, rtk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RTK_FUSED_H */
