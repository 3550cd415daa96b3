/* include/omni3d_hip.h -- C ABI of libomni3d_hip.so (gfx950 / MI355X).
 *
 * Every entry point takes raw DEVICE pointers, explicit sizes and a hipStream_t (passed as
 * void*), returns an int status (0 = OMNI_OK, 1 = bad argument, 2 = launch failure), never
 * allocates and never throws.  No torch types appear in any signature.  Each declaration cites
 * the reference interface it replaces (paths relative to the facebookresearch/omni3d checkout).
 * The reference itself has no FFI boundary (it is pure Python over detectron2 / torchvision /
 * pytorch3d); INTEGRATION.md shows the ctypes stub a maintainer would add per entry point.
 */
#ifndef OMNI3D_HIP_H
#define OMNI3D_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- IoU3D (evaluation) */

/* pytorch3d._C.iou_box3d(boxes1, boxes2) as called at
 * cubercnn/evaluation/omni3d_evaluation.py:155.  boxes1 (N,8,3), boxes2 (M,8,3) fp32 corner
 * lists in the order documented at omni3d_evaluation.py:117-142.  Writes vol (N,M) [nullable]
 * and iou (N,M).  valid1 [nullable] is an int32 (N) mask: rows with valid1[i]==0 are written as
 * zeros without being computed (box3d_overlap, omni3d_evaluation.py:151-164).  overflow
 * [nullable] is an int32 counter incremented when a pair exceeded the LDS triangle capacity. */
int omni_iou_box3d(const float* boxes1, int N, const float* boxes2, int M, const int* valid1, float* vol,
                   float* iou, int* overflow, void* stream);

/* Paired / ragged form of the same computation, for the evaluator's per-(image, category)
 * groups (Omni3Deval.computeIoU, omni3d_evaluation.py:1359-1431): pair p compares
 * boxes1[idx1[p]] with boxes2[idx2[p]]; vol [nullable] and iou have npairs entries. */
int omni_iou_box3d_pairs(const float* boxes1, const float* boxes2, const int* idx1, const int* idx2,
                         long long npairs, const int* valid1, float* vol, float* iou, int* overflow,
                         void* stream);

/* The same with the launch variant chosen by the caller: lanes_per_pair 64 | 32 | 16 = 1 | 2 | 4 pairs per wavefront over
 * full-capacity (160-triangle) LDS lists; 1000 + lanes = first pass over 96-triangle lists (more waves resident per CU), pairs
 * that outgrow them are marked and recomputed at full capacity by a second kernel of the same call; 0 = the production choice
 * (1032).  Every variant computes the same per-pair algorithm (same triangle order, same epsilon decisions); used by the parity
 * tests and by tools/bench_iou3d.py.  Replaces the same call site as above. */
int omni_iou_box3d_pairs_algo(const float* boxes1, const float* boxes2, const int* idx1, const int* idx2,
                              long long npairs, const int* valid1, float* vol, float* iou, int* overflow,
                              int lanes_per_pair, void* stream);

/* _check_coplanar (omni3d_evaluation.py:65-86) and _check_nonzero (:89-104) fused:
 * valid[i] = coplanar(i) && nonzero(i); counts [nullable, int32[2]] += {#non-coplanar, #zero}. */
int omni_box3d_validity(const float* boxes, int N, float eps_coplanar, float eps_nonzero, int* valid,
                        int* counts, void* stream);

/* Suppression of duplicate cuboids among the fixed (B, S) detection slots of the inference pass, by IoU3D and (optionally) across
 * categories (csrc/nms3d.hip).  The reference has no such step: fast_rcnn_inference_single_image
 * (cubercnn/modeling/roi_heads/fast_rcnn.py:57-143) suppresses per class and in 2D only; this stands for the `box3d_overlap` loop its
 * users run on the host afterwards.
 *   verts (B*S,8,3)   corner lists in the order of omni_iou_box3d; score (B*S); cls (B*S) int32; count (B) int32: image b uses the
 *                     slots s < count[b] (clamped to [0, S]); the slots behind it are not read
 *   iou_thr           a kept slot i removes every lower-ranked slot j with iou[b][i][j] > iou_thr (strict, as torchvision's nms)
 *   class_agnostic    0: only pairs of equal class are compared (the others have IoU 0 here)
 *   eps_coplanar, eps_nonzero   the validity test of omni_box3d_validity, taken per box
 * Two launches.  (1) the self-overlap of every image: one lane screens each pair i < j (exact 0 when j >= count[b], the classes
 * differ and class_agnostic == 0, either box is invalid, or the bounding spheres are disjoint), the others run the pair algorithm
 * of omni_iou_box3d (32 lanes per pair, full-capacity lists); the value is written to iou[b][i][j] and iou[b][j][i], the diagonal
 * is 0, every entry of iou (B,S,S) is written whatever the counts.  (2) one 256-thread workgroup per image ranks the slots by
 * descending score (ties to the lower slot; bitonic network over 64-bit keys) and walks the ranking: a candidate that has not been
 * removed is kept and removes the later candidates it overlaps by more than iou_thr.  A slot whose box is invalid (or has a
 * non-finite vertex) or whose score is not finite is kept, never suppresses and is never suppressed.  Out:
 *   keep (B,S) int32       1 for a kept slot, 0 for a removed one and for s >= count[b]
 *   order (B,S) int32      the kept slots in ASCENDING slot order, then -1: gathering by it takes rows out and reorders nothing
 *   new_count (B) int32    number of kept slots
 *   overflow (1) int32     incremented when a pair exceeded the LDS triangle capacity, as in omni_iou_box3d (the caller zeroes it)
 * No atomics in (2), no arrival order anywhere: two runs give the same bits.  S > 1024 (the LDS capacity of (2)) returns
 * OMNI_ERR_ARG before any launch; B == 0 or S == 0 launches nothing. */
int omni_nms3d(const float* verts, const float* score, const int* cls, const int* count, int B, int S, float iou_thr,
               int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* keep, int* order, int* new_count,
               int* overflow, void* stream);

/* IoU3D of two cuboids from exact geometry, in double (csrc/cuboid_exact.h, csrc/iou3d_exact.hip).  The reference has no
 * counterpart: pytorch3d's pair algorithm, which omni_iou_box3d restates, treats a triangle within 2.56 degrees of a face plane as
 * lying in it and is up to 0.3 off on near-aligned boxes.  The evaluator keeps that algorithm; this one EXTENDS the library for
 * callers that need the geometry (TEST.NMS_3D.IOU_TYPE "exact").
 *
 * omni_cuboid_fit: verts (N,8,3) float32 corner lists in the order of omni_iou_box3d -> the cuboid they are taken for, one thread
 * per box, all in double:
 *   centre (N,3)   the vertex mean
 *   axes (N,3,3)   axes[n][k] = unit axis k: the mean of the four edges parallel to it, orthonormalised (x, then y by Gram-Schmidt,
 *                  then z = +-(x cross y) on the side of the measured z)
 *   dims (N,3)     the norms of the three mean edges
 *   valid (N)      int32, 0 for an INVALID box: a non-finite vertex, a dimension <= eps_dim, or a vertex further than fit_tol x the
 *                  largest dimension from its fitted corner; centre, axes and dims of an invalid box are 0
 *   invalid        [nullable, int32[1]] += number of invalid boxes (the caller zeroes it; one integer atomic per invalid box)
 * The IoU below is DEFINED as that of the fitted cuboids: float32-rounded corners are not coplanar to better than 1e-6 of their
 * magnitude and bound no solid.  eps_dim 1e-8 and fit_tol 1e-3 are the defaults of the callers: conditions on the input.
 * omni_iou3d_exact_pairs: pair p compares fitted box idx1[p] of the first set (n1 boxes) with idx2[p] of the second (n2): vol[p] =
 * volume of the intersection, iou[p] = vol / (v1 + v2 - vol) clamped to [0, 1], v = the product of the fitted dimensions.  One
 * thread per pair: exactly 0 when either box is invalid, an index lies outside its set or the bounding spheres are disjoint;
 * otherwise every face of either box, as a rectangle in the frame of its own box, is clipped by the other box's six half-spaces
 * (Sutherland-Hodgman, <= 10 vertices, per-thread LDS lists) and vol = 1/3 sum (n . p0) area.  A signed distance within 1e-12 of
 * the pair's largest coordinate is 0; the second box's faces are clipped by OPEN half-spaces, the first's by half-spaces that are
 * closed where the two outward normals agree, so a shared face plane counts once (same side) or not at all (touching).  Never NaN.
 * No atomics: two launches give the same bits.  N == 0 / npairs == 0 launch nothing; negative sizes, a NaN or negative eps_dim /
 * fit_tol or a missing array return OMNI_ERR_ARG before anything touches the device.
 * omni_nms3d_exact: omni_nms3d with the arguments and outputs of omni_nms3d, deciding by this IoU.  Launch (1) is one THREAD per
 * slot pair i < j, written to both halves of iou (B,S,S), diagonal 0, every entry written; a slot takes part only if it passes the
 * validity test of omni_nms3d AND the fit (eps_dim 1e-8, fit_tol 1e-3), otherwise it is kept, never suppresses and is never
 * suppressed.  Launch (2) is that of omni_nms3d.  invalid (1) int32 [nullable] += number of slots s < count[b] whose fit fails
 * (the caller zeroes it); it takes the place of `overflow`: nothing here can outgrow a list. */
int omni_cuboid_fit(const float* verts, int N, double eps_dim, double fit_tol, double* centre, double* axes, double* dims, int* valid,
                    int* invalid, void* stream);
int omni_iou3d_exact_pairs(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1,
                           const double* centre2, const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1,
                           const int* idx2, long long npairs, float* vol, float* iou, void* stream);
int omni_nms3d_exact(const float* verts, const float* score, const int* cls, const int* count, int B, int S, float iou_thr,
                     int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* keep, int* order, int* new_count,
                     int* invalid, void* stream);

/* Weighted fusion of overlapping cuboids among the fixed (B, S) slots (csrc/nms3d.hip): the merge step of test-time augmentation,
 * where the slots of one image hold the detections of several views in one camera frame.  Where omni_nms3d_exact keeps the best
 * cuboid of a group and drops the rest, this turns the group into ONE cuboid: weighted-boxes-fusion carried over to oriented 3D
 * boxes.  The reference has no counterpart (detectron2's GeneralizedRCNNWithTTA merges 2D boxes by NMS).
 *   verts, score, cls, count, iou_thr, class_agnostic, eps_coplanar, eps_nonzero   as in omni_nms3d_exact
 *   aux (B*S,A)       [null when A == 0] further columns that are averaged with the geometry (2D boxes, class scores, ...)
 *   views             >= 1, the number of views the slots were gathered from
 * Two launches.  (1) the pair-matrix launch of omni_nms3d_exact, unchanged: iou (B,S,S), every entry written.  (2) one 256-thread
 * workgroup per image.  Ranking: that of omni_nms3d (descending score, ties to the lower slot); a slot takes part iff its score is
 * finite, it passes the validity test and the fit of omni_cuboid_fit (eps_dim 1e-8, fit_tol 1e-3).  Clustering: the next candidate
 * that is still live is a HEAD; its cluster is itself plus every later live candidate j with iou[head][j] > iou_thr (strict), which
 * are then dead -- greedy, not transitive.  A slot < count[b] that takes no part is a cluster of its own.  Fusion, in double, members
 * in rank order, w = max(score, 0): a member's fitted axes are first renamed to the head's -- the first permutation p of (0,1,2) in
 * lexicographic order that maximises sum_k |h_k . x_p(k)|, each axis with the sign that makes h_k . x_p(k) >= 0, the dimensions
 * permuted alike (the same body can be reported with its axes permuted and flipped) -- then centre and dimensions are the w-weighted
 * means, the axes are the orthogonal polar factor of the w-weighted mean of the aligned axis matrices (8 Newton steps
 * X <- (X + X^-T) / 2), and every aux column is the same weighted mean.  A cluster of one member, or of total weight 0, is its head
 * bit for bit (corners and aux copied).  Out, per image in DESCENDING fused score (ties to the lower head slot; a score that is not
 * finite sorts last, by slot), rows >= out_count[b] zeroed with out_head -1:
 *   cluster (B,S) int32        head slot of the cluster of slot s < count[b], -1 behind the count
 *   out_verts (B*S,8,3)        corners of the fused cuboid in the order of omni_iou_box3d, in the head's axis naming
 *   out_centre (B*S,3), out_axes (B*S,3,3) (row k = unit axis k), out_dims (B*S,3)   what omni_cuboid_fit gives for out_verts
 *                              (0 for a passed-through slot whose corners are no cuboid)
 *   out_score (B*S)            sum of the members' raw scores / max(members, views): a cuboid seen in one of T views gets score / T
 *   out_cls (B*S) int32        the head's class;  out_aux (B*S,A);  out_size (B*S) int32 members;  out_head (B*S) int32 head slot
 *   out_count (B) int32        number of clusters
 *   invalid (1) int32          [nullable] += slots < count[b] whose fit fails, as in omni_nms3d_exact (the caller zeroes it)
 * No atomics but that one, no arrival order: one thread walks a cluster, so two runs give the same bits.  S > 1024, a negative size,
 * views < 1 or a missing array return OMNI_ERR_ARG before any launch; B == 0 or S == 0 launches nothing. */
int omni_fuse3d(const float* verts, const float* score, const int* cls, const int* count, const float* aux, int B, int S, int A, int views,
                float iou_thr, int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* cluster, float* out_verts,
                float* out_centre, float* out_axes, float* out_dims, float* out_score, int* out_cls, float* out_aux, int* out_size,
                int* out_head, int* out_count, int* invalid, void* stream);

/* IoU in the bird's-eye view (csrc/bev_iou.hip): the overlap of the cuboids' footprints on the ground plane, the matching criterion
 * of AP-BEV.  The reference has no counterpart: it EXTENDS `box3d_overlap` / omni_iou_box3d_pairs with a third kind of overlap next
 * to the 2D and 3D ones of Omni3Deval.computeIoU (omni3d_evaluation.py:1359-1431).
 *
 * omni_bev_footprint: verts (N,8,3) corner lists in any order; e1, e2: an orthonormal basis of the plane orthogonal to the up
 * vector (derived on the host; up = (0,-1,0) gives e1 = x, e2 = z and an exact projection).  Out, one thread per box:
 *   poly (N,8,2)   the convex hull of the eight points (v.e1, v.e2), counter-clockwise in the (e1, e2) plane, strictly convex
 *                  (duplicate and collinear points dropped); the slots behind `count` are 0
 *   count (N)      int32 hull size, 3 .. 8; 0 for an INVALID box: a non-finite vertex, or footprint area <= eps_area
 *   area (N)       footprint area (fan from the first hull vertex); 0 for an invalid box
 *   invalid        [nullable, int32[1]] += number of invalid boxes (the caller zeroes it; one integer atomic per invalid box)
 * omni_bev_iou_pairs: iou[p] = area(P ^ Q) / (area P + area Q - area(P ^ Q)) clamped to [0, 1] for P = footprint idx1[p] of the
 * first set (n1 footprints), Q = footprint idx2[p] of the second (n2).  One thread per pair: exactly 0 when either footprint is
 * invalid, an index lies outside its set, or the bounding rectangles are disjoint; otherwise both polygons are moved to a local
 * origin (the first vertex of P) BEFORE any product is formed, P is clipped by every edge of Q (Sutherland-Hodgman, <= 16 vertices,
 * per-thread LDS lists) and the fan area taken.  Never NaN.  No atomics: two launches give the same bits.
 * N == 0 / npairs == 0 launch nothing; negative sizes, a NaN or negative eps_area, a component of e1 / e2 that is no unit vector's
 * or a missing array return OMNI_ERR_ARG before anything touches the device. */
int omni_bev_footprint(const float* verts, int N, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float eps_area,
                       float* poly, int* count, float* area, int* invalid, void* stream);
int omni_bev_iou_pairs(const float* poly1, const int* count1, const float* area1, int n1, const float* poly2, const int* count2,
                       const float* area2, int n2, const int* idx1, const int* idx2, long long npairs, float* iou, void* stream);

/* True-positive errors of the centre-distance protocol (csrc/tp_errors.hip): translation, scale and orientation error of a pair of
 * cuboids, and their averages along the recall curve (the ATE / ASE / AOE of nuScenes), for `Omni3Deval(mode="DIST")`.  The reference
 * has no counterpart.
 *
 * omni_pair_errors: pair p compares fitted box idx1[p] of the first set (n1 boxes, the arrays of omni_cuboid_fit) with idx2[p] of the
 * second (n2); err (npairs,3) double, one thread per pair, all in double:
 *   err[p][0]  trans   |d| with d = centre1 - centre2; with an up vector (upx, upy, upz), a UNIT vector, the distance in the plane
 *                      orthogonal to it, sqrt(max(0, |d|^2 - (d.up)^2)); up = (0, 0, 0) means the full 3D distance
 *   err[p][1]  scale   1 - inter / (V1 + V2 - inter), inter = prod_k min(dims1[k], dims2[k]), V = the product of the dimensions
 *   err[p][2]  orient  the geodesic angle of R = R1 R2^T (columns = the unit axes) in [0, pi] radians:
 *                      atan2(0.5 |(R32 - R23, R13 - R31, R21 - R12)|, 0.5 (trace R - 1))
 * (+inf, NaN, NaN) when either box is invalid (valid 0, or a dimension <= 0) or an index lies outside its set.  No atomics: two
 * launches give the same bits.  npairs == 0 launches nothing; negative sizes, an `up` that is neither all zeros nor of norm 1 (a NaN
 * included) or a missing array return OMNI_ERR_ARG before anything touches the device.
 * omni_eval_tp_errors: one 64-lane wave per (category k, depth range a).  order (N) / cat_off (K+1): the merge order of
 * omni_eval_accumulate; dt_match / dt_ignore (A,sumD): the slices of omni_eval_match's tables at ONE threshold; pair_row (sumD):
 * the row of err (npairs,3) that holds the pair (detection d, ground truth 0 of its group), so a matched detection's errors are row
 * pair_row[d] + dt_match[d]; npig (K,A), has_e (K), rec_thrs (R) ascending as in omni_eval_accumulate.  A detection with
 * dt_match >= 0 and dt_ignore == 0 is a true positive; at the c-th one m_c = the mean of each error over the first c; the recall
 * threshold r_j takes m_c when r_j >= min_recall and (c-1)/npig < r_j <= c/npig (the doubles and expressions of
 * omni_eval_accumulate).  tp_err (K,A,3) = the mean of the values taken, 1.0 when ground truths exist but no threshold took one;
 * tp_count (K,A) = the number of true positives.  Both are written only where has_e[k] and npig[k][a] > 0: the caller pre-fills
 * them (-1 and 0).  Sums are ballot prefixes and lane-ordered scans in double, no floating-point atomics: two launches give the same
 * bits.  K == 0 launches nothing; bad sizes, a min_recall outside [0, 1] or a missing array return OMNI_ERR_ARG before any launch. */
int omni_pair_errors(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1, const double* centre2,
                     const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1, const int* idx2,
                     long long npairs, double upx, double upy, double upz, double* err, void* stream);
int omni_eval_tp_errors(const int* order, const int* cat_off, const int* dt_match, const unsigned char* dt_ignore,
                        const long long* pair_row, const double* err, long long npairs, const int* npig, const int* has_e,
                        const double* rec_thrs, double min_recall, int K, int A, int R, int sumD, double* tp_err, int* tp_count,
                        void* stream);

/* Longitudinal-error-tolerant 3D metrics (csrc/let_iou.hip): LET-3D-AP / LET-3D-APL of Hung et al. 2022, the camera-only metric of the
 * Waymo Open Dataset, for `Omni3Deval(mode="LET")`.  The reference has no counterpart.
 *
 * omni_let_pairs: pair p takes fitted box idx1[p] of the first set (the DETECTIONS, n1 boxes, the arrays of omni_cuboid_fit; centre P)
 * and idx2[p] of the second (the GROUND TRUTHS, n2; centre G), the sensor at the origin of the coordinates, one thread per pair, all
 * in double:
 *   lon[p]  (double)  (G - P) . u with u = P / |P|: the signed longitudinal error, positive when the detection is too near
 *   aff[p]  (double)  1 - min(|lon| / T, 1) with T = max(tol_frac |G|, tol_min): the longitudinal affinity in [0, 1]
 *   iou[p]  (float)   the exact IoU3D (that of omni_iou3d_exact_pairs) of the ground truth and the detection with its centre moved
 *                     to P + lon u, the point of its line of sight closest to G, when aff > 0; exactly 0 when aff == 0
 * (0, 0, NaN) for a gated pair: either box invalid (valid 0, or a dimension <= 0), an index outside its set, or |P| <= 1e-8 (no
 * line of sight).  NaN never leaves through iou or aff.  No atomics: two launches give the same bits.  npairs == 0 launches nothing;
 * negative sizes, a tol_frac that is not finite and >= 0, a tol_min that is not finite and > 0 or a missing array return
 * OMNI_ERR_ARG before anything touches the device.
 * omni_eval_accumulate_let: one 64-lane wave per (k, a, m, t), on the arguments of omni_eval_accumulate (order, cat_off, rank,
 * dt_match / dt_ignore (A,T,sumD), npig, has_e, rec_thrs, max_dets) plus pair_row (sumD), the row of aff / lon (npairs) that holds the
 * pair (detection d, ground truth 0 of its group): the pair of a true positive is pair_row[d] + dt_match[a][t][d]; a row outside
 * [0, npairs) counts as NaN and nothing is read.  With prec_L(s) = (sum of aff over the true positives up to list position s) /
 * (tp + fp + eps), eps = 2^-52:
 *   precision_l (T,R,K,A,M)  prec_L made monotone from the right and sampled at rec_thrs exactly as `precision` is
 *   tp_affinity (T,K,A,M)    the mean aff of the true positives among the included detections (rank < max_dets[m])
 *   tp_lon      (T,K,A,M)    the mean signed lon of the same, metres
 * precision_l is written where omni_eval_accumulate writes `precision` (has_e[k] and npig[k][a] > 0), the two means where there is
 * a true positive as well: the caller pre-fills all three with -1.  Sums are ballot prefixes and lane-ordered scans in double, no
 * floating-point atomics: two launches give the same bits.  K == 0 launches nothing; bad sizes or a missing array return
 * OMNI_ERR_ARG before any launch. */
int omni_let_pairs(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1, const double* centre2,
                   const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1, const int* idx2,
                   long long npairs, double tol_frac, double tol_min, float* iou, double* aff, double* lon, void* stream);
int omni_eval_accumulate_let(const int* order, const int* cat_off, const int* rank, const int* dt_match, const unsigned char* dt_ignore,
                             const long long* pair_row, const double* aff, const double* lon, long long npairs, const int* npig,
                             const int* has_e, const double* rec_thrs, const int* max_dets, int K, int A, int M, int T, int R, int sumD,
                             double* precision_l, double* tp_affinity, double* tp_lon, void* stream);

/* ------------------------------------------------- convolution / linear (fp32 MFMA, NHWC) */

/* torch.nn.Conv2d forward as used by the DLA-34 bottom-up (cubercnn/modeling/backbone/dla.py:
 * 43-51,159-161,241-245,291-295), detectron2 FPN (dla.py:500-506) and StandardRPNHead
 * (configs/Base.yaml:49); and torch.nn.Linear (H=W=R=S=1: FastRCNNConvFCHead,
 * cubercnn/modeling/roi_heads/cube_head.py:70,108-144).
 * x is NHWC fp32 (N,H,W,C) with pixel pitch ldx floats, w is KRSC fp32, bias [nullable] (K),
 * out NHWC (N,OH,OW,K) with pitch ldo.  C and ldx must be multiples of 4.  relu != 0 fuses ReLU. */
int omni_conv2d_fwd(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int C,
                    int K, int R, int S, int stride, int pad, int ldx, int ldo, int relu, void* stream);

/* grad wrt the input of the same convolution (autograd of the call sites above):
 * dx (N,H,W,C) pitch lddx (=|+= when accumulate) from dy (N,OH,OW,K) pitch lddy. K % 4 == 0. */
int omni_conv2d_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R,
                      int S, int stride, int pad, int lddy, int lddx, int accumulate, void* stream);

/* grad wrt the weights (omni_conv2d_wgrad_algo below): dw (K,R,S,C) overwritten, or atomically accumulated into when
 * accumulate != 0 (weight gradients land directly in the flat gradient bucket).  Split-K over output pixels, fp32 atomics. */

/* The same three operations with the ALGORITHM chosen by the caller instead of by the launcher's shape heuristics
 * (cuDNN's "algo" argument; the reference reaches it through torch.backends.cudnn.benchmark, tools/train_net.py sets
 * nothing and takes the default).  tile: 0 = automatic | 1 = 128x128 | 2 = 64x64 | 3 = 128x64 | 4 = 256x32 (fwd/dgrad) or
 * 32x128 (wgrad).  splits: 0 = automatic | >= 1 = reduction splits (> 1 ends with fp32 atomics into a zeroed, dense output;
 * dgrad with accumulate != 0: on top of dx's content, any pitch -- the gradient fan-in target of functional.fanout).
 * omni_conv2d_fwd/dgrad/wgrad == the _algo form with tile = splits = 0.  Used by tools/bench_kernels.py and by tests that
 * exercise a given tile shape on a small problem; there is no process-global tuning state. */
int omni_conv2d_fwd_algo(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int C,
                         int K, int R, int S, int stride, int pad, int ldx, int ldo, int relu, int tile, int splits,
                         void* stream);
int omni_conv2d_dgrad_algo(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R,
                           int S, int stride, int pad, int lddy, int lddx, int accumulate, int tile, int splits,
                           void* stream);
int omni_conv2d_wgrad_algo(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R,
                           int S, int stride, int pad, int ldx, int lddy, int accumulate, int tile, void* stream);

/* Deterministic forms (round 4; csrc/split_reduce.h).  The reference's PyTorch-CPU path gives bit-identical results from run to
 * run; a split reduction that meets in the output through fp32 atomics does not (the order of the adds follows the order in which
 * workgroups finish).  These entry points are the three operations above with the reduction splits meeting in a caller-provided
 * workspace instead: every split stores its partial tile to `ws` (ws_floats floats), arrives at one of `ctr`'s n_ctr unsigned
 * counters (ZERO on entry, zero again on exit), and the tile's last-arriving workgroup adds the partial tiles in split order and
 * runs the normal epilogue -- bias / ReLU (fwd), overwrite or add-to-carry (dgrad, accumulate != 0), overwrite or add to the
 * gradient bucket (wgrad, accumulate != 0: plain read-modify-write, each element has one owner per launch).  No zero-fill, no
 * follow-up ReLU pass, and omni_conv2d_fwd_det emits BatchNorm statistics (stats, see omni_conv2d_fwd_stats) from split launches too.
 * plan != NULL: nothing is launched; plan[0..3] = {tile, reduction splits, counters needed (0 = not split), workspace floats
 * needed} for exactly the launch the other arguments describe, so the caller sizes `ws` / `ctr` with the launcher's own heuristics
 * (pass plan[0] / plan[1] back as tile / splits).  Replaces the same torch.nn.Conv2d / nn.Linear forward and backward calls as
 * omni_conv2d_fwd / dgrad / wgrad (dla.py:43-51, cube_head.py:70,108-163). */
int omni_conv2d_fwd_det(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int C, int K,
                        int R, int S, int stride, int pad, int ldx, int ldo, int relu, int tile, int splits, float* stats,
                        int stats_rows, int* nblk_out, float* ws, long long ws_floats, int* ctr, int n_ctr, long long* plan,
                        void* stream);

/* omni_conv2d_fwd_det for an input that is the channel concatenation of nsrc <= 6 dense NHWC tensors xs[s] (N, H, W, cs[s]),
 * cs[s] % 32 == 0, WITHOUT forming the concatenation: conv1x1(torch.cat(children, 1)) of the DLA Root
 * (cubercnn/modeling/backbone/dla.py:166-172).  1 x 1, stride 1, no padding; out (N, H, W, K) with pixel pitch ldo.  Same tiles,
 * splits, epilogues and bit-identical results as the single-tensor entry on the concatenated input.  xs / cs are HOST arrays.
 * ctr == NULL && plan == NULL: non-deterministic form (split reductions meet through atomics). */
int omni_conv2d_fwd_multi_det(const void* const* xs, const int* cs, int nsrc, const float* w, const float* bias, float* out, int N, int H,
                              int W, int K, int ldo, int relu, int tile, int splits_req, float* stats, int stats_rows, int* nblk_out,
                              float* ws, long long ws_floats, int* ctr, int n_ctr, long long* plan, void* stream);
int omni_conv2d_dgrad_det(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int lddy, int lddx, int accumulate, int tile, int splits, float* ws,
                          long long ws_floats, int* ctr, int n_ctr, long long* plan, void* stream);
int omni_conv2d_wgrad_det(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int ldx, int lddy, int accumulate, int tile, float* ws, long long ws_floats,
                          int* ctr, int n_ctr, long long* plan, void* stream);

/* OPT-IN EXPERIMENT, round 6 (csrc/gemm_split.hip; SURVEY.md section 7 "3 x bf16 split"): the batched NT GEMM of omni_gemm_batched
 * -- out[b] (M x N) = A[b] (M x K) B[b] (N x K)^T, fp32 in / out, K % 32 == 0 -- on the bf16 matrix cores from an error-free split of
 * the operands into 2 (terms = 3 products) or 3 (terms = 6) bf16 planes, fp32 accumulation.  Never selected by default: the measured
 * path multiplies fp32 operands (v_mfma_f32_32x32x2_f32). */
int omni_gemm_batched_split(const float* A, const float* B, float* out, int batch, int M, int N, int K, int terms, void* stream);
/* Round 6 (csrc/dgrad_s2.hip): data gradient of the 3x3 / stride-2 / pad-1 convolutions that open every DLA level and ResNet stage
 * (cubercnn/modeling/backbone/dla.py:43-51, 186-215; autograd of nn.Conv2d).  dx (N, H, W, C) [pixel pitch lddx] (=, or += when
 * accumulate != 0: a gradient fan-in target) from dy (N, (H-1)/2+1, (W-1)/2+1, K) [pitch lddy] and w (K, 3, 3, C); C, K multiples
 * of 32.  One workgroup computes all four parity classes of a 16 x 16 dx tile from one staged dy tile: dy is read once, every dx
 * element written once by its owner -- deterministic, no atomics, no zero-fill. */
int omni_conv2d_s2_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int lddy, int lddx,
                         int accumulate, void* stream);
/* omni_conv2d_wgrad_det for an input that is the channel concatenation of nsrc <= 6 dense NHWC tensors (omni_conv2d_fwd_multi_det):
 * dw (K, 1, 1, sum cs) = dy^T x of the DLA Root's 1 x 1 convolution (dla.py:166-172) without the concatenated copy; cs[s] % 4 == 0,
 * xs / cs HOST arrays, dy (N, H, W, K) with pixel pitch lddy.  Bit-identical to the single-tensor entry on the concatenated input.
 * ctr == NULL && plan == NULL: non-deterministic form. */
int omni_conv2d_wgrad_multi_det(const void* const* xs, const int* cs, int nsrc, const float* dy, float* dw, int N, int H, int W, int K,
                                int lddy, int accumulate, int tile, float* ws, long long ws_floats, int* ctr, int n_ctr, long long* plan,
                                void* stream);

/* ------------------------------------------------------- BatchNorm / pooling / FPN (NHWC) */

/* nn.BatchNorm2d in training mode (+ fused ReLU and residual add): cubercnn/modeling/backbone/
 * dla.py:46-66 (BasicBlock), :162-172 (Root), :214 (project), :244,294 (conv levels).
 * x, y, residual [nullable]: NHWC fp32 with P = N*H*W pixels, C % 4 == 0, C <= 1024.
 * running_mean/var [nullable] updated with `momentum` (unbiased var) like F.batch_norm.
 * Outputs kept for backward: mean_rstd (2C), scale_shift (2C).  ws: >= 2C*258 doubles scratch.
 * Backward: dy = grad wrt y; dres [nullable] = grad wrt residual; ws >= 2C*258 doubles, coef 3C floats scratch.  relu: 0 = none;
 * 1 = mask dy by y > 0, y = the forward output; 2 = layers without residual: `y` points at the forward pass's scale_shift (2C floats)
 * and the mask is recomputed as x * scale + shift > 0, the output tensor is not read.
 * Every variant sits behind explicit arguments.  partial [nullable] = [nblk][2][C] statistics rows already written by the producer of x
 * (forward) / of dy (backward); NULL = a reduction pass runs first (ws as above).  ldy / lddy / ldc: pixel pitches in floats of y, dy
 * and res_carry (0 or C = dense; a DLA Root child, dla.py:171, is written into / read from its channel slice of the concatenated
 * tensor).  fuse_rows: with <= fuse_rows partial rows and C % 16 == 0 the finalize is folded into the apply launch -- every workgroup
 * owns 16 channels of a pixel chunk and sums the rows of those channels itself in the finalize kernel's order: same bits, one
 * dependent launch less (0 = always the separate finalize launch). */
int omni_bn_fwd_algo(const float* x, const float* partial, int nblk, const float* gamma, const float* beta, const float* residual,
                     float* y, long long ldy, float* running_mean, float* running_var, float* mean_rstd, float* scale_shift,
                     double* ws, int P, int C, float eps, float momentum, int relu, int fuse_rows, void* stream);
int omni_bn_bwd_algo(const float* x, const float* dy, long long lddy, const float* y, const float* gamma, const float* mean_rstd,
                     const float* partial, int nblk, float* dx, float* dres, const float* res_carry, long long ldc, float* dgamma,
                     float* dbeta, double* ws, float* coef, int P, int C, int relu, int accumulate_param_grads, int fuse_rows,
                     void* stream);

/* eval-mode / frozen BatchNorm (solver/build.py:71-76 freeze_bn): y = relu?(x*scale+shift(+res)). */
int omni_bn_apply(const float* x, const float* scale_shift, const float* residual, float* y, int P, int C,
                  int relu, void* stream);

/* frozen BatchNorm WITH gradients: the eval-mode BatchNorm2d of a training pass after freeze_bn (tools/train_net.py:150-151, :297-298;
 * cubercnn/solver/build.py:71-76), MODEL.USE_BN False (cubercnn/config/config.py:82).  Forward y = relu?(x * s + t (+ residual)),
 * s = gamma * rsqrt(running_var + eps), t = beta - running_mean * s made inside the launch from the live tensors (no host cache: a
 * captured graph reads the current parameters on every replay); the same bits as omni_bn_apply with the eval-mode (scale, shift).
 * Backward, g = dy masked by the ReLU (relu 0: none | 1: y > 0, y = the forward output | 2: x * s + t > 0 recomputed, forward
 * without residual, y unused): dx = g * s, dres = g + res_carry [dres, res_carry nullable; pitch ldc], dbeta = sum g,
 * dgamma = sum g * (x - running_mean) * rsqrt(running_var + eps) -- written, or added (accumulate_param_grads) to dgamma / dbeta
 * (both NULL: not computed).  dy with pixel pitch lddy.  One pass + a fixed-order finalize, no atomics: run-to-run identical.
 * ws >= 2 * C * 512 floats.  Running statistics are never written. */
int omni_bn_frozen_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, const float* residual, float* y, int P, int C, int relu, void* stream);
int omni_bn_frozen_bwd(const float* x, const float* dy, long long lddy, const float* y, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps, float* dx, float* dres, const float* res_carry,
                       long long ldc, float* dgamma, float* dbeta, float* ws, long long ws_floats, int P, int C, int relu,
                       int accumulate_param_grads, void* stream);

/* nn.MaxPool2d(2, stride=2) (dla.py:209) forward / backward, NHWC. */
int omni_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int omni_maxpool2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* Grouped convolution `nn.Conv2d(C, K, R, stride, pad, groups=G, bias=False)` of DLA's BottleneckX (cubercnn/modeling/backbone/
 * dla.py:112-153): x (N,H,W,C), w (K,R,S,C/G), out / dy (N,OH,OW,K); C/G and K/G multiples of 4.  One launch of the implicit-GEMM
 * kernels per group on channel slices (pixel pitch C / K). */
int omni_grouped_conv2d_fwd(const float* x, const float* w, float* out, int N, int H, int W, int C, int K, int R, int S, int stride,
                            int pad, int groups, void* stream);
int omni_grouped_conv2d_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int S, int stride,
                              int pad, int groups, void* stream);
int omni_grouped_conv2d_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int S, int stride,
                              int pad, int groups, void* stream);

/* Depthwise convolution `nn.Conv2d(C, C, R, padding=pad, stride=stride, groups=C, bias=False)` of torchvision's mnasnet1_0
 * (lifted by cubercnn/modeling/backbone/mnasnet.py:14-17): R in {3, 5}, stride in {1, 2}; x (N,H,W,C), w (R,R,C) tap-major,
 * y / dy (N,OH,OW,C), dw (R,R,C) overwritten. */
int omni_dwconv_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int R, int stride, int pad, void* stream);
int omni_dwconv_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int R, int stride, int pad, void* stream);
int omni_dwconv_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int R, int stride, int pad, void* stream);

/* nn.AvgPool2d(2, stride=2) of torchvision densenet121's transitions (cubercnn/modeling/backbone/densenet.py:14-15, 27-30)
 * forward / backward, NHWC; dy (N, H/2, W/2, C) -> dx (N, H, W, C). */
int omni_avgpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int omni_avgpool2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* F.max_pool2d(x, kernel_size=1, stride=2) (dla.py:474, resnet.py:55): y[n,oh,ow]=x[n,2oh,2ow]. */
int omni_subsample2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int omni_subsample2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* detectron2 FPN top-down step: out = lateral + F.interpolate(top, 2.0, "nearest"); and the
 * gradient wrt `top` (2x2 block sums). */
int omni_upsample2_add(const float* lat, const float* top, float* out, int N, int H, int W, int C,
                       void* stream);
int omni_upsample2_bwd(const float* dout, float* dtop, int N, int H, int W, int C, void* stream);

/* Gradient fan-in ("carry") forms of four backward kernels.  An activation with several consumers -- the input of a DLA Tree
 * (max-pool + first block, cubercnn/modeling/backbone/dla.py:204-222), a block output that is the next block's input, its residual
 * and a Root child (:60-66, :171-173), an FPN top-down map (detectron2 FPN.forward, built at dla.py:500-506), an FPN output read
 * by the RPN head and by ROIAlign (cubercnn/modeling/roi_heads/roi_heads.py:267,362) -- has a gradient that is the SUM of its
 * consumers' gradients; autograd forms that sum with one elementwise add kernel per extra consumer.  Here the consumer that runs
 * later reads what the earlier ones produced (`carry`: NHWC, same extent as the output, pixel pitch ldc floats -- a whole tensor or a
 * channel slice of the Root's concatenated gradient; ldc >= channels, ldc % 4 == 0, 16-byte aligned) and writes the sum:
 *   omni_wino_out_carry      y = A^T M A + carry                 (Winograd data gradient, tile as omni_wino_out)
 *   omni_bn_bwd_algo         dres = masked dy + res_carry        (res_carry nullable)
 *   omni_maxpool2_bwd_carry  dx = routed dy + carry              (carry nullable; H, W even when given)
 *   omni_upsample2_bwd_carry dtop = 2x2 block sums + carry       (carry nullable)
 *   omni_subsample2_bwd_carry dx = carry + dy at the even pixels (the p6 = p5[::2, ::2] level; one pass instead of fill + scatter + add)
 * The implicit-GEMM data gradient takes the same role through omni_conv2d_dgrad(accumulate = 1, lddx = the carry's pitch).
 * omni_bn_bwd_algo / omni_maxpool2_bwd_carry also read their OUTPUT gradient dy with a pixel pitch lddy (same constraints): a
 * Root child with no other consumer gets its slice of the concatenated gradient without a copy. */
int omni_wino_out_carry(const float* M, const float* carry, long long ldc, float* y, int N, int H, int W, int K, int tile, void* stream);
int omni_maxpool2_bwd_carry(const float* x, const float* dy, long long lddy, const float* carry, long long ldc, float* dx, int N, int H,
                            int W, int C, void* stream);
int omni_subsample2_bwd_carry(const float* dy, const float* carry, long long ldc, float* dx, int N, int H, int W, int C, void* stream);
int omni_upsample2_bwd_carry(const float* dout, const float* carry, long long ldc, float* dtop, int N, int H, int W, int C,
                             void* stream);

/* GeneralizedRCNN.preprocess_image (called at cubercnn/modeling/meta_arch/rcnn3d.py:46,87):
 * uint8 planar (N,3,H,W) -> fp32 NHWC (N,PH,PW,4), (v-mean)/std, channel 3 and padding = 0. */
int omni_preprocess(const unsigned char* img, float* out, int N, int H, int W, int PH, int PW, float m0,
                    float m1, float m2, float s0, float s1, float s2, void* stream);
/* The same for a batch staged into fixed-size slots: image_hw (N,2) device ints = the valid height / width of image n inside its
 * H x W slot; everything outside is zero padding like the reference's ImageList.from_tensors of the real sizes
 * (rcnn3d.py:46 -> detectron2 ImageList).  Lets one captured training step serve every batch of a size bucket
 * (configs/Base.yaml:10-13 draws a new short edge per image; cubercnn/solver/autoreplay.py). */
int omni_preprocess_masked(const unsigned char* img, const int* image_hw, float* out, int N, int H, int W, int PH, int PW,
                           float m0, float m1, float m2, float s0, float s1, float s2, void* stream);
/* Round 6: the same from N <= 64 SEPARATE images (imgs: HOST array of N device pointers to planar uint8 (3, H, W) images) -- the
 * `torch.stack` of ImageList.from_tensors folded into the read; image_hw nullable. */
int omni_preprocess_multi(const void* const* imgs, const int* image_hw, float* out, int N, int H, int W, int PH, int PW, float m0,
                          float m1, float m2, float s0, float s1, float s2, void* stream);

/* ----------------------------------------------------------- index-exact selection kernels */

/* Row-wise sorted top-k (descending; equal keys -> lower index first).  Stands in for
 * `logits.sort(descending=True)[:k]` of detectron2 find_top_rpn_proposals (RPN configured at
 * configs/Base.yaml:49-54) and for torch.multinomial (== top-k of w / Exp(1)) at
 * cubercnn/modeling/proposal_generator/rpn.py:318,322.  Element (r,i) = keys[r*pitch + i*estride].
 * out_val / out_idx: (rows, k); slots >= min(k,n) hold -inf / -1.  k <= 8192. */
int omni_topk_rows(const float* keys, int rows, int n, long long pitch, int estride, int k, float* out_val,
                   int* out_idx, void* stream);
/* The same for `nseg` (<= 8) column segments of every row in one launch: the per-FPN-level pre-NMS top-k of
 * detectron2 find_top_rpn_proposals (one sort per level and image upstream).  seg_off / seg_n are HOST int arrays;
 * out_val / out_idx: (rows, nseg, k), indices relative to the segment start. */
int omni_topk_segments(const float* keys, int rows, long long pitch, int estride, int nseg, const int* seg_off,
                       const int* seg_n, int k, float* out_val, int* out_idx, void* stream);

/* Greedy NMS (torchvision.ops.nms semantics: suppress iff IoU > thr, areas (x2-x1)*(y2-y1)) for Q
 * independent score-sorted problems; detectron2 batched_nms = one problem per (image, level) /
 * (image, class): RPN [upstream], cubercnn/modeling/roi_heads/fast_rcnn.py:105.
 * boxes (Q,nmax,4); counts [nullable] (Q); valid [nullable] (Q,nmax); keep (Q,nmax) int32 0/1;
 * mask_ws: Q*nmax*ceil(nmax/64) 64-bit words scratch. nmax <= 8192. */
int omni_nms_sorted(const float* boxes, const int* counts, const int* valid, int Q, int nmax, float iou_thr,
                    unsigned long long* mask_ws, int* keep, void* stream);
/* The same, and the scan also writes masked (Q,nmax) = keep ? scores : -inf (every element), the input of the post-NMS
 * top-k of find_top_rpn_proposals.  scores / masked are nullable, together: omni_nms_sorted forwards here with both null. */
int omni_nms_sorted_masked(const float* boxes, const int* counts, const int* valid, int Q, int nmax, float iou_thr,
                           unsigned long long* mask_ws, int* keep, const float* scores, float* masked, void* stream);

/* ---------------------------------------------- RPN / ROI-head box logic (index-exact parts) */

/* detectron2 pairwise_iou (mode 0) / pairwise_ioa (mode 1): cubercnn/modeling/proposal_generator/
 * rpn.py:62,100; roi_heads/roi_heads.py:881,892.  out (N, M). */
int omni_pairwise_iou(const float* boxes1, int N, const float* boxes2, int M, int mode, float* out, void* stream);

/* RPNWithIgnore.label_and_sample_anchors, matching half (rpn.py:62-75; omni_rpn_match_draw below) = pairwise_iou + detectron2
 * Matcher(thr, labels, allow_low_quality) + per-GT best anchor, for a batch of B images.
 * anchors (A,4); gt: concatenated valid GT boxes (G,4) with gt_off (B+1); expo (B,A) Exp(1) variates.
 * Outputs (B,A): matched_val, matched_idx (GT index inside the image), match_label int8,
 * key_pos / key_neg = (iou+eps)/E for the positive / negative candidates (-inf elsewhere) whose
 * top-k is the IoU-weighted multinomial of rpn.py:318,322; gt_best_idx (G); gt_best_bits (G) scratch. */

/* Second half (rpn.py:79-105): labels (B,A) int8 in {-1,0,1} from the sampled top-k lists, forced
 * best-anchor positives and ignore regions (ign (Gi,4), ign_off (B+1)).  counts (B,2) [nullable]. */
int omni_rpn_finalize_labels(const float* anchors, int A, int B, const int* gt_off, const float* ign,
                             const int* ign_off, const signed char* match_label, const int* gt_best_idx,
                             const float* pos_val, const int* pos_idx, const float* neg_val, const int* neg_idx,
                             int kpos, int kneg, int batch_per_image, float ignore_thresh, signed char* labels,
                             int* counts, void* stream);

/* RPN head tensors: level_ptrs is a HOST array of nlev device pointers to (B, hw_l, 16) fp32
 * [3 logits | 12 deltas | pad], level_hw a HOST int array.  Gathers the logits into (B, A). */
int omni_rpn_gather_logits(const void* const* level_ptrs, const int* level_hw, int nlev, int B, float* logits,
                           void* stream);

/* The two 1x1 convolutions of detectron2's StandardRPNHead (objectness_logits: nn.Conv2d(256, 3, 1), anchor_deltas:
 * nn.Conv2d(256, 12, 1); configs/Base.yaml:49, reached from cubercnn/modeling/proposal_generator/rpn.py:129-135) over ALL FPN levels
 * in one launch per direction, as one 16-wide product per pixel: y[p] = [3 logits | 12 deltas | 0] (the layout above).
 * t / y / dy / dt: HOST arrays of nlev (<= 8) device pointers -- t_l (P_l, 256) fp32 NHWC = relu(conv(x_l)), y_l / dy_l (P_l, 16),
 * dt_l (P_l, 256); pix: HOST array of P_l = B * H_l * W_l; w_obj (3, 256), w_del (12, 256), biases (3), (12).
 *   fwd    y_l = t_l . [w_obj | w_del | 0]^T + [b_obj | b_del | 0]                 (fp32 MFMA 16x16x4, operands straight from HBM)
 *   dgrad  dt_l = dy_l . [w_obj | w_del | 0], zeroed where t_l <= 0 when relu_mask != 0 (the ReLU backward of the shared conv)
 *   wgrad  dw_obj, db_obj, dw_del, db_del [each nullable] = (accumulate == 0) or += the sums over every pixel of every level;
 *          partial = scratch of partial_rows (>= 1; 512 fills the chip) * (15 * 256 + 16) floats; fixed summation order, no atomics. */
int omni_rpn_head16_fwd(const void* const* t, const long long* pix, int nlev, const float* w_obj, const float* b_obj,
                        const float* w_del, const float* b_del, const void* const* y, void* stream);
int omni_rpn_head16_dgrad(const void* const* dy, const void* const* t, const long long* pix, int nlev, const float* w_obj,
                          const float* w_del, int relu_mask, const void* const* dt, void* stream);
int omni_rpn_head16_wgrad(const void* const* dy, const void* const* t, const long long* pix, int nlev, float* partial,
                          int partial_rows, float* dw_obj, float* db_obj, float* dw_del, float* db_del, int accumulate, void* stream);

/* RPNWithIgnore.losses with OBJECTNESS_UNCERTAINTY "IoUness" (rpn.py:129-204, 206-273): sums (6 doubles)
 * = [sum BCE*t, sum L1*t, #pos, #neg, sum sigmoid(pos), sum sigmoid(non-pos)]. */
int omni_rpn_loss_fwd(const void* const* level_ptrs, const int* level_hw, int nlev, int B, const float* anchors,
                      const signed char* labels, const int* matched_idx, const float* gt, const int* gt_off,
                      double* sums, void* stream);
int omni_rpn_loss_bwd(const void* const* level_ptrs, const void* const* dlevel_ptrs, const int* level_hw, int nlev,
                      int B, const float* anchors, const signed char* labels, const int* matched_idx,
                      const float* gt, const int* gt_off, const float* g_cls, const float* g_loc, float inv_norm,
                      void* stream);

/* The same with OBJECTNESS_UNCERTAINTY "none" (rpn.py:181-195, detectron2's own RPN losses): objectness BCE against the 0 / 1
 * labels over every sampled anchor, unweighted L1 on the foreground deltas; same sums layout. */
int omni_rpn_loss_plain_fwd(const void* const* level_ptrs, const int* level_hw, int nlev, int B, const float* anchors,
                            const signed char* labels, const int* matched_idx, const float* gt, const int* gt_off,
                            double* sums, void* stream);
int omni_rpn_loss_plain_bwd(const void* const* level_ptrs, const void* const* dlevel_ptrs, const int* level_hw, int nlev,
                            int B, const float* anchors, const signed char* labels, const int* matched_idx,
                            const float* gt, const int* gt_off, const float* g_cls, const float* g_loc, float inv_norm,
                            void* stream);

/* Both of the above with the localisation term MODEL.RPN.BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA name instead of L1 (plain == 0:
 * IoUness, rpn.py:258-271 -- smooth-L1 with beta, IoU-weighted, every other type is OMNI_ERR_ARG as it is a ValueError there;
 * plain != 0: 'none', detectron2's _dense_box_regression_loss called at rpn.py:181-195 -- also giou / diou / ciou (fvcore) on
 * Box2BoxTransform.apply_deltas(deltas, anchor), weights (1,1,1,1), dw / dh bounded by scale_clamp, summed over the positives).
 * reg_type: 0 smooth_l1, 1 giou, 2 diou, 3 ciou; beta >= 0 (< 1e-5: L1).  Same sums layout, same gradient arguments. */
int omni_rpn_reg_loss_fwd(const void* const* level_ptrs, const int* level_hw, int nlev, int B, const float* anchors,
                          const signed char* labels, const int* matched_idx, const float* gt, const int* gt_off, int plain,
                          int reg_type, float beta, float scale_clamp, double* sums, void* stream);
int omni_rpn_reg_loss_bwd(const void* const* level_ptrs, const void* const* dlevel_ptrs, const int* level_hw, int nlev,
                          int B, const float* anchors, const signed char* labels, const int* matched_idx,
                          const float* gt, const int* gt_off, int plain, int reg_type, float beta, float scale_clamp,
                          const float* g_cls, const float* g_loc, float inv_norm, void* stream);

/* detectron2 RPN._decode_proposals + Boxes.clip + nonempty filter of find_top_rpn_proposals, applied
 * to the selected per-level top-k anchors only.  slot_level (Ktot), idx (B,Ktot), image_hw (B,2) are
 * device arrays; boxes (B,Ktot,4), valid (B,Ktot) out. */
int omni_rpn_decode(const void* const* level_ptrs, const int* level_hw, int nlev, int B, int Ktot,
                    const int* slot_level, const int* idx, const float* anchors, const int* image_hw,
                    float scale_clamp, float min_size, float* boxes, int* valid, void* stream);

/* Post-NMS glue of find_top_rpn_proposals (detectron2; the `keep[:post_nms_topk]` step of the RPN configured in
 * /root/reference/configs/Base.yaml:49-54).  omni_rpn_mask_scores: masked (n) = keep ? scores : -inf, the input of the
 * post-NMS ranking.  omni_rpn_collect: boxes (B,N,4), top_v / top_i (B,P) = that ranking (sorted, -inf / -1 padded)
 * -> prop (B,P,4) (zeros behind the real ones), count (B). */
int omni_rpn_mask_scores(const float* scores, const int* keep, long long n, float* masked, void* stream);
int omni_rpn_collect(const float* boxes, const float* top_v, const int* top_i, int B, int N, int P, float* prop,
                     int* count, void* stream);

/* ROIHeads3D.label_and_sample_proposals (roi_heads.py:862-929; omni_roi_sample_draw below): append GT, Matcher(iou_thr), ignore
 * regions, IoU-weighted sampling of <= nfg_max foreground + background up to batch_per_image.
 * expo (B, 2048).  Outputs (B, batch_per_image): boxes, class (num_classes = bg, -2 = padding),
 * global GT row, matched IoU; counts (B,2). */
/* Round 6 forms of the two subsampling steps: expo == NULL draws the Exp(1) variates INSIDE the kernel (csrc/philox.h: Philox4x32-10
 * keyed by draw_state[0] = seed, counter (element, row, draw_state[1]); the last workgroup to take its ticket advances
 * draw_state[1]; ticket: one zeroed int32) -- replaces `Tensor.exponential_()` + torch's graph-safe generator bookkeeping, six
 * launches per step for the randomness of detectron2 `subsample_labels` (rpn.py:41-127 / roi_heads.py:862-929 call sites).
 * omni_roi_sample_draw also emits out_row (out_gt with -1 -> 0, the `clamp(min=0)` of the loss call sites) and contiguous copies
 * of the first `first` slots per image (the cube head's ROIs: roi_heads.py:341-362). */
int omni_rpn_match_draw(const float* anchors, int A, const float* gt, const int* gt_off, int B, int G, float thr_lo,
                        float thr_hi, int l0, int l1, int l2, int allow_low_quality, const float* expo, long long* draw_state,
                        int* ticket, float eps, float* matched_val, int* matched_idx, signed char* match_label, int* gt_best_bits,
                        int* gt_best_idx, float* key_pos, float* key_neg, void* stream);
int omni_roi_sample_draw(const float* prop_boxes, const int* prop_count, int B, int pmax, const float* gt, const int* gt_cls,
                         const int* gt_off, const float* ign, const int* ign_off, const float* expo, long long* draw_state, int* ticket,
                         float iou_thr, float ignore_thresh, float eps, int num_classes, int batch_per_image, int nfg_max,
                         int append_gt, float* out_boxes, int* out_cls, int* out_gt, float* out_iou, int* out_counts, int* out_row,
                         int first, float* first_boxes, int* first_cls, int* first_row, void* stream);

/* ----------------------------------------------------------------------------- ROIAlign */

/* detectron2 assign_boxes_to_levels (ROIPooler, canonical 224 / level 4). */
int omni_roi_levels(const float* rois, int R, int min_level, int max_level, float canonical_size,
                    int canonical_level, int* levels, void* stream);

/* detectron2 ROIPooler + torchvision roi_align(aligned=True, sampling_ratio=0): box pooler
 * (roi_heads.py:267) and cube pooler (roi_heads.py:166-171,362).  level_ptrs/level_hw/level_scale are
 * HOST arrays; features (B,H_l,W_l,C) NHWC; out (R,P,P,C). */
int omni_roi_align_fwd(const void* const* level_ptrs, const int* level_hw, const float* level_scale, int nlev,
                       const float* rois, const int* batch_idx, const int* levels, int R, int P, int C,
                       float* out, void* stream);
/* Round 6: torchvision roi_align with its `aligned` switch exposed: aligned = 0 is detectron2's POOLER_TYPE "ROIAlign" (no half-pixel
 * shift, ROI sides of at least one pixel), 1 = "ROIAlignV2" (cubercnn/modeling/roi_heads/roi_heads.py:166-171 passes
 * MODEL.ROI_BOX_HEAD.POOLER_TYPE / MODEL.ROI_CUBE_HEAD.POOLER_TYPE through to detectron2's ROIPooler).  Any P; the backward adds into
 * dlevel_ptrs with fp32 atomics (the caller zeroes them). */
int omni_roi_align_fwd_mode(const void* const* level_ptrs, const int* level_hw, const float* level_scale, int nlev,
                            const float* rois, const int* batch_idx, const int* levels, int R, int P, int C, int aligned, float* out,
                            void* stream);
int omni_roi_align_bwd_mode(const void* const* dlevel_ptrs, const int* level_hw, const float* level_scale, int nlev,
                            const float* rois, const int* batch_idx, const int* levels, int R, int P, int C, int aligned,
                            const float* dout, void* stream);
/* Round 6: POOLER_TYPE "ROIPool" = torchvision.ops.roi_pool as detectron2's ROIPooler applies it level by level (the reference passes
 * MODEL.ROI_BOX_HEAD.POOLER_TYPE / MODEL.ROI_CUBE_HEAD.POOLER_TYPE through: cubercnn/modeling/roi_heads/roi_heads.py:166-171).
 * out and argmax (R, P, P, C); argmax = h * W + w of the first maximum inside the ROI's image and level, -1 for an empty bin (out 0).
 * The backward adds dout at the argmax pixels with fp32 atomics (the caller zeroes dlevel_ptrs). */
int omni_roi_pool_fwd(const void* const* level_ptrs, const int* level_hw, const float* level_scale, int nlev, const float* rois,
                      const int* batch_idx, const int* levels, int R, int P, int C, float* out, int* argmax, void* stream);
int omni_roi_pool_bwd(const void* const* dlevel_ptrs, const int* level_hw, const float* level_scale, int nlev, const int* batch_idx,
                      const int* levels, int R, int P, int C, const float* dout, const int* argmax, void* stream);
/* Round 6: forward that also writes the first `first` ROIs of every block of `per_image` to out2 ((R / per_image) * first, P, P, C) --
 * the box head's and the cube head's pooled features in one pass (roi_heads.py:166-171, 267, 362), no slice copy. */
int omni_roi_align_fwd2(const void* const* level_ptrs, const int* level_hw, const float* level_scale, int nlev,
                        const float* rois, const int* batch_idx, const int* levels, int R, int P, int C, float* out,
                        float* out2, int per_image, int first, void* stream);
int omni_roi_align_bwd(const void* const* dlevel_ptrs, const int* level_hw, const float* level_scale, int nlev,
                       const float* rois, const int* batch_idx, const int* levels, int R, int P, int C,
                       const float* dout, void* stream);
/* The same with two gradient tensors (P == 7): dout (R,7,7,C) [nullable] and dout2 ((R / per_image) * first, 7, 7, C) [nullable] for
 * the first `first` ROIs of every block of `per_image` (the cube head's ROIs are a prefix of the box head's in one shared pass). */
int omni_roi_align_bwd2(const void* const* dlevel_ptrs, const int* level_hw, const float* level_scale, int nlev,
                        const float* rois, const int* batch_idx, const int* levels, int R, int P, int C,
                        const float* dout, const float* dout2, int per_image, int first, void* stream);
/* Deterministic form (round 4; P == 7, R <= 4096, B = images): the OUTPUT owns the sum -- one workgroup per 8 x 4 pixel tile of a
 * (level, image), all channels: its four waves deal out the ROIs that touch the tile (wave s: entries s, s + 4, ... of the list in
 * ascending ROI index) and meet in wave order, so an element's value depends on the inputs alone; every element of dlevel_ptrs[l]
 * is written exactly once (OVERWRITES: no zero-fill by the caller), no atomics: two runs are bit-identical.
 * C <= 256, B <= 255.  ws: scratch for per-ROI footprint records (plan != NULL: plan[3] = floats needed, nothing is launched);
 * ctr / n_ctr are not used by this kernel.  Same call site and gradient arguments as omni_roi_align_bwd2. */
int omni_roi_align_bwd_det(const void* const* dlevel_ptrs, const int* level_hw, const float* level_scale, int nlev, int B,
                           const float* rois, const int* batch_idx, const int* levels, int R, int P, int C, const float* dout,
                           const float* dout2, int per_image, int first, float* ws, long long ws_floats, int* ctr, int n_ctr,
                           long long* plan, void* stream);

/* ------------------------------------------------------------------- box-head / cube losses */

/* FastRCNNOutputs.losses (cubercnn/modeling/roi_heads/fast_rcnn.py:145-260) on the fused prediction
 * tensor pred (R, ldp) = [K+1 logits | 4K deltas].  sums (7 doubles). */
int omni_box_loss_fwd(const float* pred, int ldp, int R, int K, const int* cls, const float* prop, const float* gt,
                      const int* gt_row, float wx, float wy, float ww, float wh, double* sums, void* stream);
int omni_box_loss_bwd(const float* pred, int ldp, int R, int K, const int* cls, const float* prop, const float* gt,
                      const int* gt_row, float wx, float wy, float ww, float wh, const double* sums,
                      const float* g_cls, const float* g_reg, float* dpred, void* stream);

/* The same with the regression term MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA name instead of L1: smooth-L1 with
 * beta (cubercnn/modeling/roi_heads/fast_rcnn.py:245-252), or giou / diou / ciou (fvcore) of
 * Box2BoxTransform.apply_deltas(GT-class deltas, proposal) against the ground-truth box, summed over the foreground rows
 * (detectron2 FastRCNNOutputLayers.box_reg_loss; the reference's own box head stops at fast_rcnn.py:253-254 for these).
 * reg_type: 0 smooth_l1, 1 giou, 2 diou, 3 ciou; beta >= 0 (< 1e-5: L1); scale_clamp bounds dw / dh (IoU types).  Same sums. */
int omni_box_reg_loss_fwd(const float* pred, int ldp, int R, int K, const int* cls, const float* prop, const float* gt,
                          const int* gt_row, float wx, float wy, float ww, float wh, int reg_type, float beta,
                          float scale_clamp, double* sums, void* stream);
int omni_box_reg_loss_bwd(const float* pred, int ldp, int R, int K, const int* cls, const float* prop, const float* gt,
                          const int* gt_row, float wx, float wy, float ww, float wh, int reg_type, float beta,
                          float scale_clamp, const double* sums, const float* g_cls, const float* g_reg, float* dpred,
                          void* stream);

/* FastRCNNOutputLayers.predict_boxes_for_gt_classes (detectron2), called at cubercnn/modeling/roi_heads/roi_heads.py:276-289
 * (MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES): out (R,4) = Box2BoxTransform.apply_deltas of each row's GT-class deltas
 * (class clamped to [0, K-1]; cls < 0 copies the proposal) on its proposal box, unclipped. */
int omni_box_decode_gt_class(const float* pred, int ldp, int R, int K, const int* cls, const float* prop, float wx, float wy,
                             float ww, float wh, float scale_clamp, float* out, void* stream);

/* ROIHeads3D._forward_cube decode + losses (cubercnn/modeling/roi_heads/roi_heads.py:374-768) on the fused cube-head
 * outputs head (F, ldh) = [xy 2K | z K*bins (bin*K + class) | dims 3K | pose Pn*K | uncert K (if confidence)],
 * Pn = 6 / 4 / 3 for POSE_TYPE 6d / quaternion / euler (cube_head.py:118-136,175-192), bins = max(CLUSTER_BINS, 1).
 * mode = MODEL.ROI_CUBE_HEAD configuration: bits 0-1 Z_TYPE (0 direct, 1 sigmoid, 2 log, 3 clusters), bits 2-3 dimensions
 * (0 priors 'exp', 1 priors 'sigmoid', 2 DIMS_PRIORS_ENABLED False), bits 4-5 POSE_TYPE (0 6d, 1 quaternion, 2 euler),
 * bit 6 ALLOCENTRIC_POSE, bit 7 VIRTUAL_DEPTH, bit 8 CHAMFER_POSE, bit 9 INVERSE_Z_WEIGHT, bit 10 USE_CONFIDENCE > 0,
 * bit 11 LOSS_W_JOINT > 0, bit 12 DISENTANGLED_LOSS False (configs/Base.yaml = 0xDC0).
 * zscales (K, bins): 2D-scale prior of every depth cluster (roi_heads.py:123-130), zstats (K, bins, 2): its depth mean / std
 * (:133-143); null when bins == 1 / Z_TYPE is not 'clusters'.  Bit 12 needs dimensions = 2: the reference's own entangled
 * dimension loss cannot be evaluated with priors (roi_heads.py:620-622 divides an (n,3) by an (n,2,3) tensor).
 * w_*: MODEL.ROI_CUBE_HEAD.LOSS_W_{DIMS,POSE,XY,Z,JOINT}, used for the logged `Cube/total_3D_loss` (:651-695). */
int omni_cube_loss_fwd(const float* head, int ldh, int F, int K, int mode, int bins, const float* zscales, const float* zstats,
                       const float* boxes, const int* cls, const int* img,
                       const float* Ks, const float* v2r, const float* priors, const float* gt3d,
                       const float* gtpose, const int* gt_row, float w_dims, float w_pose, float w_xy, float w_z, float w_joint,
                       float* vals, float* jac, float* red, void* stream);
int omni_cube_loss_bwd(const float* vals, const float* jac, const float* red, const float* gk, const int* cls,
                       const float* boxes, int F, int K, int mode, int bins, const float* zscales, int ldh, float* dhead,
                       void* stream);
/* inference outputs (roi_heads.py:771-819): cube3d (F,9), pose (F,9), verts (F,24). */
int omni_cube_decode(const float* head, int ldh, int F, int K, int mode, int bins, const float* zscales, const float* zstats,
                     const float* boxes, const int* cls, const int* img,
                     const float* Ks, const float* v2r, const float* ratio, const float* priors, float* cube3d,
                     float* pose, float* verts, void* stream);
/* util.get_cuboid_verts_faces (cubercnn/util/math_util.py:116-219): box3d (n,6), R (n,9) -> (n,24). */
int omni_cuboid_corners(const float* box3d, const float* R, int n, float* verts, void* stream);

/* ------------------------------------------- BatchNorm statistics from the producing kernel's epilogue
 * The conv -> BatchNorm pairs of the bottom-up (cubercnn/modeling/backbone/dla.py:46-66,162-172,214,244; torchvision
 * BasicBlock via resnet.py:17-27): the convolution / Winograd output transform / stem kernel also writes per-workgroup
 * partial sums and sums of squares of its output, stats [rows][2][K] floats, so training-mode BatchNorm skips its own
 * statistics pass (omni_bn_fwd_algo with `partial` = finalize + apply).  *nblk_out = partial rows written; 0 means "not produced"
 * (split reduction chosen, buffer too small, unsupported channel count) and the caller passes partial = NULL to omni_bn_fwd_algo. */
int omni_conv2d_fwd_stats(const float* x, const float* w, float* out, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int ldx, int ldo, float* stats, int stats_rows, int* nblk_out, void* stream);
int omni_wino_out_stats(const float* M, float* y, int N, int H, int W, int K, int tile, float* stats, int stats_rows,
                        int* nblk_out, void* stream);
/* The same idea in the backward pass: the Winograd data-gradient transform of the convolution ABOVE a BatchNorm(+ReLU) writes that
 * BatchNorm's output gradient dy, and emits the per-workgroup partial sums (sum dz, sum dz * xhat) its backward pass starts with
 * (dz = dy masked by x * scale + shift > 0 when scale_shift != NULL); omni_bn_bwd_algo with `partial` = finalize + apply on those
 * rows.  *nblk_out == 0: not produced, omni_bn_bwd_algo runs its own reduction pass. */
int omni_wino_out_bn_bwd_stats(const float* M, float* y, int N, int H, int W, int K, int tile, const float* bn_x,
                               const float* mean_rstd, const float* scale_shift, float* stats, int stats_rows, int* nblk_out,
                               void* stream);
int omni_stem_conv_fwd_stats(const float* x, const float* w, float* out, int N, int H, int W, int C, int K, int R, int ldx,
                             int ldo, float* stats, int stats_rows, int* nblk_out, void* stream);

/* ---------------------------------------------------------------- GEMM engine (csrc/gemm_engine.hip)
 * The cuBLAS calls behind nn.Linear (detectron2 FastRCNNConvFCHead; cubercnn/modeling/roi_heads/cube_head.py:70,108-163),
 * behind 1x1 nn.Conv2d (FPN laterals, DLA roots / projections, cubercnn/modeling/backbone/dla.py:159-161,214) and the point
 * GEMMs of the Winograd path, forward / data gradient / weight gradient:
 *   form 0 "NT": C = A (M x K) * B (N x K)^T     form 1 "NN": C = A (M x K) * B (K x N)     form 2 "TN": C = A (K x M)^T * B (K x N)
 * batch problems at element strides stride_a/b/c; pitches lda/ldb/ldc; splits > 1 or accumulate != 0 => fp32 atomics into C
 * (zeroed by the caller unless accumulating); bias (N) / ReLU on the direct-store path.  tile: 1 = 256x128, 2 = 128x128.
 * workgroups: persistent workgroups walking the (problem, tile, split) list (0 = one per CU). */
int omni_gemm_engine(const float* A, const float* B, float* C, const float* bias, int form, int batch, int M, int N, int K,
                     int lda, int ldb, int ldc, long long stride_a, long long stride_b, long long stride_c, int splits,
                     int relu, int accumulate, int tile, int workgroups, void* stream);
/* Deterministic form (round 4, csrc/split_reduce.h; same call sites): the parts of a cut tile -- splits > 1, or the left-over tiles
 * of the balanced split (splits == -1) -- meet in `ws` (ws_floats floats) and are summed in part order by the tile's last-arriving
 * workgroup (ctr: n_ctr zeroed unsigned counters, left zeroed), which applies bias / ReLU and overwrites C or, accumulate != 0,
 * adds to it with a plain read-modify-write; the caller zeroes nothing.  plan != NULL: plan[0..3] = {0, parts per cut tile,
 * counters needed, workspace floats needed}, nothing is launched. */
int omni_gemm_engine_det(const float* A, const float* B, float* C, const float* bias, int form, int batch, int M, int N, int K,
                         int lda, int ldb, int ldc, long long stride_a, long long stride_b, long long stride_c, int splits,
                         int relu, int accumulate, int tile, int workgroups, float* ws, long long ws_floats, int* ctr, int n_ctr,
                         long long* plan, void* stream);

/* dst (cols, rows) = src (rows, cols)^T, contiguous row-major fp32.  Brings the fc1-class weights (K_out x C_in) into the
 * (C_in x K_out) layout the data gradient of torch.nn.Linear (FastRCNNConvFCHead fc1, cube_head.py:70) multiplies in the
 * engine's fastest ("NT") form. */
int omni_transpose2d(const float* src, float* dst, int rows, int cols, void* stream);

/* ---------------------------------------------------------------- batched inference
 * fast_rcnn_inference / fast_rcnn_inference_single_image (cubercnn/modeling/roi_heads/fast_rcnn.py:33-116) for all images
 * of a batch with fixed shapes.  pred (B*P, ld) = [K+1 logits | 4K deltas]; rois (B*P,4); count (B); image_hw (B,2).
 *  omni_det_scores: probs (B*P,K) softmax, boxes (B*P,K,4) decoded (Box2BoxTransform weights wx..wh) and clipped,
 *    scores (B, P*K) = prob where the row is valid (finite, p < count) and prob > score_thresh, else -inf;
 *  [omni_topk_rows over scores -> vals / idx (B, cap), stable descending]
 *  omni_det_nms_boxes: candidate boxes + class * (max coordinate + 1) (detectron2 batched_nms) -> nms_boxes (B,cap,4), valid;
 *  [omni_nms_sorted -> keep (B, cap)]
 *  omni_det_compact: the first topk kept candidates per image -> out_box (B,topk,4), out_score, out_cls, out_roi, out_count. */
int omni_det_scores(const float* pred, int ld, const float* rois, const int* count, const int* image_hw, int B, int P, int K,
                    float wx, float wy, float ww, float wh, float score_thresh, float* scores, float* probs, float* boxes,
                    void* stream);
int omni_det_nms_boxes(const float* boxes, const float* vals, const int* idx, int B, int PK, int K, int cap, float* nms_boxes,
                       int* valid, void* stream);
int omni_det_compact(const int* keep, const int* valid, const float* vals, const int* idx, const float* boxes, int B, int PK,
                     int K, int cap, int topk, float* out_box, float* out_score, int* out_cls, int* out_roi, int* out_count,
                     void* stream);

/* ------------------------------------------------------------------ input pipeline
 * detectron2 T.ResizeShortestEdge -> ResizeTransform.apply_image = PIL Image.resize(BILINEAR) on the uint8 image, and
 * RandomFlip (horizontal), as configured by cubercnn/data/dataset_mapper.py:25-27 + configs/Base.yaml:10-13.  Bit-exact
 * with Pillow's 8-bit resampling: the fixed-point coefficient rows are built by the caller (omni3d_amd/kernels/resize.py,
 * the arithmetic of Pillow's precompute_coeffs) -- bounds (n_out, 2) = [first source index, count], kk (n_out, ksize) int32.
 * src (planes, H, W) -> dst (planes, HO, WO), tmp = planes*H*WO bytes scratch; flip != 0 mirrors the output columns. */
int omni_resize_bilinear_u8(const unsigned char* src, unsigned char* dst, unsigned char* tmp, int planes, int H, int W,
                            int HO, int WO, const int* bounds_h, const int* kk_h, int ksize_h, const int* bounds_v,
                            const int* kk_v, int ksize_v, int flip, void* stream);
/* Training augmentations (csrc/augment.hip): INPUT.CROP and INPUT.COLOR_JITTER.
 * omni_pil_bilinear_coeffs: the tables above for in_size -> out_size, built on the device, one thread per output index: the double
 * arithmetic of kernels/resize.py::pil_bilinear_coeffs in its order, contraction off -- bit-equal to it for every size pair.  The
 * whole ksize row is written, zeros included.  ksize must be 2 * ceil(max(in_size / out_size, 1)) + 1, else OMNI_ERR_ARG. */
int omni_pil_bilinear_coeffs(int in_size, int out_size, int* bounds, int* kk, int ksize, void* stream);
/* omni_resize_bilinear_u8 of the window src[:, y0:y0+ch, x0:x0+cw] of the full (planes, H, W) image -> dst (planes, HO, WO), read
 * in place through the image's pitch: no copy of the window, nothing outside it is read.  tmp = planes*ch*WO bytes; the tables are
 * those of (cw -> WO) and (ch -> HO).  ch == HO skips the vertical pass, cw == WO the horizontal one; an identity size is a windowed
 * mirror (flip) or a windowed copy kernel.  A window not inside [0, W) x [0, H) or a non-positive extent returns OMNI_ERR_ARG
 * before any launch. */
int omni_crop_resize_u8(const unsigned char* src, unsigned char* dst, unsigned char* tmp, int planes, int H, int W, int x0, int y0,
                        int ch, int cw, int HO, int WO, const int* bounds_h, const int* kk_h, int ksize_h, const int* bounds_v,
                        const int* kk_v, int ksize_v, int flip, void* stream);
/* Brightness, contrast and saturation of a (3, H, W) image in place, in integers: weights wb / wc / ws with 12 fractional bits
 * (4096 = 1.0), each in [0, 16384] else OMNI_ERR_ARG; c_red = plane of red (0 RGB, 2 BGR), green is plane 1.  >> is arithmetic,
 * clamp is to [0, 255]:
 *   v1 = clamp((wb*v + 2048) >> 12)
 *   S = sum of v1 over the N = 3*H*W values, M8 = (256*S + N/2) / N;  v2 = clamp((wc*256*v1 + (4096-wc)*M8 + 2^19) >> 20)
 *   g8 = 77*R2 + 150*G2 + 29*B2;                                      v3 = clamp((ws*256*v2 + (4096-ws)*g8 + 2^19) >> 20)
 * A weight of 4096 is the identity; all three at 4096 launch nothing.  sum: one device unsigned long long, zeroed and filled here
 * when wc != 4096 (one 64-bit integer atomic per workgroup, same bits every run) and read by the apply pass on the device. */
int omni_color_jitter_u8(unsigned char* img, int H, int W, int wb, int wc, int ws, int c_red, unsigned long long* sum, void* stream);
/* INPUT.CAMERA_ROTATION (csrc/warp.hip): a projective warp with bilinear sampling.  src (planes, H, W) -> dst (planes, HO, WO), both
 * contiguous, not overlapping; m = 9 HOST doubles, row-major, mapping an output pixel to a source pixel; fill = `planes` HOST bytes.
 * Both are read at the call and passed to the kernel by value.  One double-precision projective map per pixel, every product and
 * sum rounded on its own in the order written (no contraction), then integers -- the same bytes on the host and on every device.
 * For output row i, column j:
 *   xd = j + 0.5, yd = i + 0.5
 *   X = (m0*xd + m1*yd) + m2,  Y = (m3*xd + m4*yd) + m5,  D = (m6*xd + m7*yd) + m8
 *   r = 1.0 / D,  u = X*r,  v = Y*r
 *   if !(u >= 0 && u <= W && v >= 0 && v <= H): out[p] = fill[p] in every plane p (a NaN fills as well)
 *   su = u - 0.5, sv = v - 0.5, x0 = floor(su), y0 = floor(sv)
 *   a = (int)((su - x0)*256.0 + 0.5), b = (int)((sv - y0)*256.0 + 0.5)            both in [0, 256]
 *   x1 = x0 + 1, y1 = y0 + 1, all four indices clamped into the image (edge replication)
 *   top = s[y0][x0]*(256-a) + s[y0][x1]*a,  bot = s[y1][x0]*(256-a) + s[y1][x1]*a
 *   out = (top*(256-b) + bot*b + 32768) >> 16                                      at most 255*65536 + 32768 < 2^31
 * OMNI_ERR_ARG, and nothing launched: a null pointer, a size <= 0, planes > 4, overlapping src / dst ranges, an entry of m that is not
 * finite, D <= 0 at one of the corners (0,0), (WO,0), (0,HO), (WO,HO) of the output rectangle (D is affine: positive at the corners,
 * positive all over it). */
int omni_warp_homography_u8(const unsigned char* src, unsigned char* dst, int planes, int H, int W, int HO, int WO, const double* m,
                            const unsigned char* fill, void* stream);

/* ---------------------------------------------------------------------------- optimizer */

/* torch.optim.SGD step (cubercnn/solver/build.py:49-56, tools/train_net.py:250) over a flat bucket; the gradient is
 * read as grad * grad_scale (1/world after a summing all-reduce: DDP's averaging, tools/train_net.py:449-454). */
int omni_sgd_step(float* param, const float* grad, float* momentum_buf, long long n, float lr, float momentum,
                  float dampening, float weight_decay, int nesterov, int first_step, float grad_scale,
                  const float* skip_flag, void* stream);
/* torch.optim.Adam / AdamW (+ amsgrad) as built by cubercnn/solver/build.py:58-65 (eps 1e-2, betas (0.9, 0.999), the parameter
 * groups' lr / weight decay), single-tensor form, over one group's range of the flat buckets.  decoupled: 0 Adam (L2 into the
 * gradient), 1 AdamW (p *= 1 - lr wd).  max_exp_avg_sq: null or the amsgrad running maximum.  step: device float = number of this
 * update (bias corrections); omni_adam_tick advances it once per optimizer step unless skip_flag is set. */
int omni_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long long n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int decoupled, const float* step, float grad_scale,
                   const float* skip_flag, void* stream);
int omni_adam_tick(float* step, const float* skip_flag, void* stream);
/* SOLVER.CLIP_GRADIENTS: detectron2's maybe_add_gradient_clipping, which cubercnn/solver/build.py:68 applies last -- inside
 * optimizer.step() (tools/train_net.py:250) torch.nn.utils.clip_grad_norm_ / clip_grad_value_ on EACH parameter on its own, ~230
 * per-tensor calls -- over the flat gradient bucket.  tiles (ntiles x 3 long long) = [parameter index, first bucket element,
 * element count], sorted by first element, covering exactly every parameter's own elements (no padding); ptab (nparams x 2 long
 * long) = [first tile, tile count] of each parameter.  Pointers are bucket BASES; the tiles address into them.
 *  omni_clip_norm_partials: partial[t] = sum |g|^p over tile t (max |g| for norm_type = inf), one workgroup per tile.
 *  omni_clip_norm_coef: norm[k] = grad_scale * (parameter k's partials summed in tile order)^(1/p), coef[k] = min(max_norm /
 *    (norm[k] + 1e-6), 1).  NaN propagates into norm and coef (also for inf); grad_scale as in omni_sgd_step.  No atomics.
 *  omni_sgd_step_clipped / omni_adam_step_clipped: omni_sgd_step / omni_adam_step over the tiles [t0, t1) of one group's range,
 *    the gradient read as g * grad_scale * coef[k] (clip_mode 1 = norm) or clamp(g * grad_scale, -clip_value, clip_value)
 *    (clip_mode 2 = value, NaN stays NaN) before weight decay / momentum / moments.  The clipped gradient is not written back. */
int omni_clip_norm_partials(const float* grad, const long long* tiles, int ntiles, float norm_type, double* partial, void* stream);
int omni_clip_norm_coef(const double* partial, const long long* ptab, int nparams, float norm_type, float max_norm, float grad_scale,
                        float* norm, float* coef, void* stream);
int omni_sgd_step_clipped(float* param, const float* grad, float* momentum_buf, const long long* tiles, int t0, int t1, int clip_mode,
                          const float* coef, float clip_value, float lr, float momentum, float dampening, float weight_decay,
                          int nesterov, int first_step, float grad_scale, const float* skip_flag, void* stream);
int omni_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                           const long long* tiles, int t0, int t1, int clip_mode, const float* coef, float clip_value, float lr,
                           float beta1, float beta2, float eps, float weight_decay, int decoupled, const float* step,
                           float grad_scale, const float* skip_flag, void* stream);
/* The loop's divergence guard (tools/train_net.py:157-285: allreduce_dict :186, rolling-loss test :194-215, skip / step
 * :245-253, retry decision :258-270) around ONE small all-reduce.  vec (n + 2): [n loss scalars | sum | non-finite-gradient flag];
 * omni_guard_pre writes the sum, the caller all-reduces vec over the ranks (sum), omni_guard_post averages by `world`, updates
 * state (3) = [rolling loss (NaN = unset), iterations_success, iterations_explode], writes skip (1) for omni_sgd_step and
 * out (n + 3) = [skipped, retry, total, n reduced losses], and clears the flag. */
int omni_guard_pre(float* vec, int n, void* stream);
int omni_guard_post(float* vec, int n, int world, float stabilize, float half_period, float tolerance, float gamma, float* state,
                    float* skip, float* out, void* stream);
/* ---- round 6 (csrc/glue.hip): the scalar-sized ATen launches around the losses and the loop, one launch each.
 * omni_scale_vec: out[i] = (float)(src[i * stride] * coef[i] / max(*denom, denom_min)), i < n <= 16, in double, rounded once --
 *   `loss * weight`, `loss_sum / max(count, 1)` (detectron2 fast_rcnn.py losses(); cubercnn/modeling/roi_heads/roi_heads.py:745-768);
 *   src double when src_f64 else float, stride 0 = one broadcast scalar; coef: n HOST doubles or NULL; denom: device scalar or NULL.
 * omni_sum_vectors: out[0] / out[1] / out[2] = sum of the first nfirst vectors / of the rest / of all -- `sum(loss_dict.values())`
 *   (tools/train_net.py:180) split at the backward-stage boundary; vecs / lens: nvec <= 16 HOST entries (device pointers, lengths).
 * omni_guard_gather: vec[i] = *scalars[i], vec[n] = their sum -- the stacking of tools/train_net.py:186 + omni_guard_pre.
 * omni_bump_counters: *counters[i] += delta (nn.BatchNorm2d's num_batches_tracked of every layer; HOST array of device pointers).
 * omni_zero: zero-fill as a kernel node (optimizer.zero_grad() of the flat gradient bucket, tools/train_net.py:217). */
int omni_scale_vec(const void* src, int src_f64, int stride, const double* coef, const void* denom, double denom_min, int n, float* out,
                   void* stream);
int omni_sum_vectors(const void* const* vecs, const int* lens, int nvec, int nfirst, float* out, void* stream);
int omni_guard_gather(const void* const* scalars, int n, float* vec, void* stream);
int omni_bump_counters(const void* const* counters, int n, long long delta, void* stream);
int omni_zero(void* p, long long nbytes, void* stream);
/* the isnan/isinf gradient scan of tools/train_net.py:222-233 as one pass; flag[0] = 1 if any. */
int omni_nonfinite_any(const float* grad, long long n, float* flag, void* stream);

/* backward of the ReLU fused into conv / linear epilogues, and the bias gradient (per-channel sum
 * of dy over P pixels; ws 2C*258 doubles scratch).  autograd of the nn.Conv2d / nn.Linear call sites.  accumulate: 0 = overwrite | 1 = add (small tensors: fp32 atomics) | 3 = add
 * deterministically (partial rows + fixed-order finalize, round 4). */
int omni_relu_bwd(const float* dy, const float* y, float* dz, long long n, void* stream);
int omni_bias_grad(const float* dy, int P, int C, float* db, double* ws, int accumulate, void* stream);

/* nn.MaxPool2d(3, stride=2, padding=1) of the torchvision ResNet stem (cubercnn/modeling/backbone/resnet.py:34,52),
 * NHWC forward / backward (gather form, deterministic). */
int omni_maxpool3s2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int omni_maxpool3s2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* ------------------------------------------------- Winograd F(2x2,3x3) path for wide 3x3 / s1 / p1 convolutions
 * (detectron2 FPN output convs built at cubercnn/modeling/backbone/dla.py:500-506 and StandardRPNHead.conv,
 * configs/Base.yaml:49 -- nn.Conv2d(256, 256, 3, padding=1) upstream).  H and W even, channels % 4 == 0.
 * T = N*H/2*W/2 tiles.  V / M / dM: [16][T][channels]; U: [16][K][C]; U' (rotated, channel-transposed filter): [16][C][K]. */
/* tile = 2: F(2x2,3x3), P = 16 points;  tile = 4: F(4x4,3x3), P = 36 points, H and W multiples of 4.  T = N*(H/tile)*(W/tile);
 * the [16] above reads [P]. */
int omni_wino_in(const float* x, float* V, int N, int H, int W, int C, int tile, void* stream);
int omni_wino_out(const float* M, const float* bias, float* y, int N, int H, int W, int K, int relu, int tile, void* stream);
int omni_wino_dy(const float* dy, float* dM, int N, int H, int W, int K, int tile, void* stream);
/* omni_wino_weights for n <= 48 filters in ONE launch (the weights are fixed during a step: every filter transform of the forward pass
 * at once).  g / U / U_flip: HOST arrays of device pointers (U[i] / U_flip[i] nullable, not both); K / C / tile: HOST int arrays. */
int omni_wino_weights_multi(const void* const* g, const void* const* U, const void* const* U_flip, const int* K, const int* C,
                            const int* tile, int n, void* stream);
/* backward: dM (as omni_wino_dy) and V_dy (as omni_wino_in of dy) from one read of dy */
int omni_wino_dy_in(const float* dy, float* dM, float* Vd, int N, int H, int W, int K, int tile, void* stream);
int omni_wino_weights(const float* g, float* U /*nullable*/, float* U_flip /*nullable: U'*/, int K, int C, int tile, void* stream);
int omni_wino_dweights(const float* dU, float* dg, int K, int C, int accumulate, int tile, void* stream);
/* n <= 16 of them in one launch, each ADDED into its gradient view; sources naming the same dg (the RPN's shared convolution: one
 * weight gradient per FPN level) are added in the order given, as the separate launches would */
int omni_wino_dweights_multi(const void* const* dU, const void* const* dg, const int* K, const int* C, const int* tile, int n,
                             void* stream);
/* `batch` independent dense GEMMs in one launch (the 16 Winograd points):
 * fwd: out[b](M,K) = x[b](M,C) * w[b](K,C)^T;  wgrad: dw[b](K,C) = dy[b](M,K)^T * x[b](M,C) (overwrites dw). */
/* algo: 0 = automatic | 1 = persistent workgroups walking the (problem, tile) list (`workgroups` of them, multiple of 8,
 * 0 = default; C % 32 == 0) | 2 = one 128x128 tile per workgroup | 3 = one 64x64 tile per workgroup | 4 = 64x64 tiles with
 * 2-4 slabs of buffer-load prefetch in flight (short reductions: the small-map point GEMMs; C % 64 == 0) */
int omni_gemm_batched_fwd_algo(const float* x, const float* w, float* out, int batch, int M, int C, int K, int algo,
                               int workgroups, void* stream);
/* algo: 0 = automatic | 1 = the implicit-GEMM weight-gradient tiles (128x128 / 64x64) | 2 = 64x64 tiles with 4 slabs of
 * buffer-load prefetch in flight (short reductions).  The call site is the Winograd-domain weight
 * gradient of torch.nn.Conv2d's backward (dla.py:43-51). */
int omni_gemm_batched_wgrad_algo(const float* x, const float* dy, float* dw, int batch, int M, int C, int K, int algo,
                                 void* stream);
/* deterministic form (see omni_conv2d_fwd_det): the row splits of the Winograd-domain weight gradient meet in `ws` in split order */
int omni_gemm_batched_wgrad_det(const float* x, const float* dy, float* dw, int batch, int M, int C, int K, int algo, float* ws,
                                long long ws_floats, int* ctr, int n_ctr, long long* plan, void* stream);
/* n <= 16 such weight-gradient GEMMs of different shapes in ONE launch (round 4: all the Winograd layers whose data gradients a
 * backward stage has produced; each alone is a latency-bound launch on 256 CUs).  Problem i: dw[i] (batch[i], K[i], C[i]) =
 * dy[i] (batch[i], M[i], K[i])^T x[i] (batch[i], M[i], C[i]); tiles, row splits and (ctr != NULL) the ordered split reduction are
 * those of omni_gemm_batched_wgrad_det(algo 2) on that problem alone -- bit-identical to n separate calls.  ws / ctr hold the
 * problems' regions back to back; plan: [0] = 2, [1] = 0, [2] = counters, [3] = workspace floats of the whole call. */
int omni_gemm_batched_wgrad_multi(const void* const* x, const void* const* dy, const void* const* dw, const int* batch, const int* M,
                                  const int* C, const int* K, int n, float* ws, long long ws_floats, int* ctr, int n_ctr,
                                  long long* plan, void* stream);

/* Direct convolution for the full-resolution, few-channel DLA-34 stem layers (cubercnn/modeling/backbone/dla.py:241-247):
 * out (N,H,W,16) = conv(x (N,H,W,C), w (16,R,R,C)), stride 1, padding R/2; (C, R) = (4, 7) [base_layer, image padded
 * 3 -> 4 channels] or (16, 3) [level0; also its data gradient with the rotated, channel-transposed filter]. */
int omni_stem_conv_fwd(const float* x, const float* w, float* out, int N, int H, int W, int C, int K, int R, int ldx, int ldo,
                       void* stream);
/* Round 5: the data gradients of the full-resolution stem layers on the same design (input halo + whole filter in LDS, MFMA 16x16x4).
 * omni_stem_conv_dgrad: 3x3 16 -> 16 stride 1 (level0, dla.py:246-247) from the layer's FORWARD filter -- the 180-degree rotation and
 * the channel transposition happen while the filter is staged.  omni_stem_conv_s2_dgrad: 3x3 stride 2 pad 1, 16 -> 32 (level1,
 * dla.py:248-249): dx (N,H,W,16) from dy (N,(H-1)/2+1,(W-1)/2+1,32); parity classes of the strided gradient inside one launch. */
int omni_stem_conv_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int lddy, int lddx,
                         void* stream);
int omni_stem_conv_s2_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int lddy, int lddx,
                            void* stream);
/* Its weight gradient: dw (16,R,R,C) = (accumulate == 0) or += sum over pixels of dy (N,H,W,16) (x) x (N,H,W,C). */
int omni_stem_conv_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int ldx, int lddy,
                         int accumulate, void* stream);
/* deterministic form (round 4): per-workgroup partial filter gradients in `ws` (plan != NULL: plan[3] = floats needed, nothing
 * launched), added in a fixed order by a second launch; same call site as omni_stem_conv_wgrad */
int omni_stem_conv_wgrad_det(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int ldx, int lddy,
                             int accumulate, float* ws, long long ws_floats, long long* plan, void* stream);
/* Round 6: the first layer (cubercnn/modeling/backbone/dla.py:241-245, 7x7 3 -> 16) on the 4-channel padded image with the filter
 * as the model holds it -- w / dw (16, R, R, cw), cw = 3 < C = 4: no padded copy of the filter, no slice + add of its gradient.
 * stats [nullable] as omni_stem_conv_fwd_stats; the weight gradient is the deterministic form (ws / plan as omni_stem_conv_wgrad_det). */
int omni_stem_conv_fwd_cw(const float* x, const float* w, int cw, float* out, int N, int H, int W, int C, int K, int R, int ldx, int ldo,
                          float* stats, int stats_rows, int* nblk_out, void* stream);
int omni_stem_conv_wgrad_det_cw(const float* x, const float* dy, float* dw, int cw, int N, int H, int W, int C, int K, int R, int ldx,
                                int lddy, int accumulate, float* ws, long long ws_floats, long long* plan, void* stream);
/* The stride-2 member of the family (round 4): dw (32,3,3,16) from x (N,H,W,16) and dy (N,H/2,W/2,32), H and W even -- the
 * weight gradient of DLA-34's level1 convolution (cubercnn/modeling/backbone/dla.py:291-295; torch.nn.Conv2d backward).
 * deterministic != 0: ws / plan as omni_stem_conv_wgrad_det; 0: fp32 atomics into dw. */
int omni_stem_conv_s2_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int ldx, int lddy,
                            int accumulate, int deterministic, float* ws, long long ws_floats, long long* plan, void* stream);

/* Greedy detection <-> ground-truth matching of Omni3Deval.evaluateImg (cubercnn/evaluation/omni3d_evaluation.py:1433-1551,
 * 3D mode) for all (image, category) groups x A depth ranges x T IoU thresholds.  ious: ragged (D_g, G_g) matrices at
 * iou_off[g] (rows = detections in descending score order); dt_off / gt_off: (ngroups + 1) prefix offsets; max_gt <= 1024.
 * Out: dt_match (A,T,sumD) matched gt index within the group (original order) or -1; gt_match (A,T,sumG) matched dt index or
 * -1; dt_ignore (A,T,sumD); gt_order (A,sumG) the stable ignore-last order; gt_ig (A,sumG) `_ignore` per original gt. */
int omni_eval_match(const float* ious, const long long* iou_off, const int* dt_off, const int* gt_off, const int* gt_ignore,
                    const float* gt_range, const float* dt_range, const float* areas, const double* thrs, int ngroups, int A,
                    int T, int sumD, int sumG, int max_gt, int* dt_match, int* gt_match, unsigned char* dt_ignore, int* gt_order,
                    unsigned char* gt_ig, void* stream);

/* Omni3Deval.accumulate (omni3d_evaluation.py:1172-1313).  order (N): all detections sorted by (category, descending score)
 * (stable); cat_off (K+1); rank (sumD): position of a detection in its image's score-sorted list; dt_match / dt_ignore:
 * outputs of omni_eval_match; npig (K,A) non-ignored ground truths; has_e (K); rec_thrs (R); max_dets (M).
 * precision / scores (T,R,K,A,M) and recall (T,K,A,M): doubles, pre-filled with -1 by the caller. */
int omni_eval_accumulate(const int* order, const int* cat_off, const int* rank, const double* score, const int* dt_match,
                         const unsigned char* dt_ignore, const int* npig, const int* has_e, const double* rec_thrs,
                         const int* max_dets, int K, int A, int M, int T, int R, int sumD, double* precision, double* recall,
                         double* scores, void* stream);

/* omni_eval_accumulate over many workgroups per list (csrc/eval_accumulate_par.hip), for lists too long for one wave: with useCats = 0
 * there is one list of all detections.  The arguments of omni_eval_accumulate, plus `block` = the elements of `order` per workgroup (a
 * multiple of 64) and a workspace of the caller of at least omni_eval_accumulate_par_workspace(...) bytes, 8-byte aligned, contents
 * irrelevant before and after.  No list may be longer than sumD.  Three plain launches on `stream` (per block: counts; the prefix of the
 * counts and the block's largest precision; the carry of the later blocks and the backward sweep); no atomics, no grid-wide barrier.
 * precision / recall / scores are bit for bit those of omni_eval_accumulate, the -1 of the caller and the 0.0 fills included.
 * OMNI_ERR_ARG before any launch: the conditions of omni_eval_accumulate, a block that is no positive multiple of 64, a missing,
 * misaligned or short workspace, K x A x M x T x ceil(sumD / block) >= 2^31. */
int omni_eval_accumulate_par_workspace(int K, int A, int M, int T, int sumD, int block, long long* bytes);
int omni_eval_accumulate_par(const int* order, const int* cat_off, const int* rank, const double* score, const int* dt_match,
                             const unsigned char* dt_ignore, const int* npig, const int* has_e, const double* rec_thrs,
                             const int* max_dets, int K, int A, int M, int T, int R, int sumD, int block, void* workspace,
                             long long workspace_bytes, double* precision, double* recall, double* scores, void* stream);

/* The image-level bootstrap of Omni3Deval.accumulate (csrc/eval_bootstrap.hip): AP and recall of B resampled data sets from one set of
 * match tables, for `Omni3Deval.bootstrap`.  The reference has no counterpart.  Replicate b is the row weights[b] (I) of non-negative
 * image multiplicities; its result is by definition what omni_eval_accumulate gives on the data set that holds image i weights[b][i]
 * times (copies adjacent in the image order): a detection d counts as weights[b][det_img[d]] consecutive identical entries of the merge
 * order.  max_weight: the largest weight of the table; a weight outside [0, max_weight] counts as 0.
 * omni_eval_bootstrap_counts: the groups are the (image, category) groups in (category, image) order: grp_off (K+1) their ranges per
 * category, grp_img (G) the index of the group's image in [0, I), grp_npig (G,A) the group's non-ignored ground truths per range,
 * sumG an upper bound of every column sum of grp_npig (the number of ground truths).  npig_b (B,K,A) = the weighted sums over the groups
 * of the category, has_e_b (B,K) = 1 when a group of the category has a positive weight.  One 64-lane wave per (b, k), integer sums.
 * omni_eval_bootstrap: order, cat_off, rank, dt_match / dt_ignore (A,T,sumD), rec_thrs, max_dets as in omni_eval_accumulate; det_img
 * (sumD) the index of a detection's image in [0, I) (a detection with another index has weight 0).  Out, doubles pre-filled with -1 by
 * the caller: ap (B,T,K,A,M) = (the sum over r of the replicate's `precision`) / R, ar (B,T,K,A,M) its `recall`; both stay -1 where
 * omni_eval_accumulate writes nothing (has_e_b 0 or npig_b 0).  ar is bit for bit the recall of the duplicated data set; the R
 * precisions are bit for bit its precisions, summed in the order of the backward walk (not in ascending r: ap differs from that sum by
 * rounding only).  One workgroup per (k, a, m, t) and 64 replicates: the list is staged in LDS once for all of them.  No atomics: two
 * launches, and any split of the replicates over several calls, give the same bits.
 * Both return OMNI_ERR_ARG before any launch on B <= 0, a non-positive A / M / T / R, a negative K / sumD / G / sumG / I / max_weight, a
 * missing array, I >= 2^29, and when a weighted count could reach 2^31: sumD x max_weight >= 2^31 (omni_eval_bootstrap) or sumG x
 * max_weight >= 2^31 (omni_eval_bootstrap_counts).  K == 0 launches nothing; sumD == 0 is valid (ap = ar = 0 where there is ground truth). */
int omni_eval_bootstrap_counts(const int* grp_off, const int* grp_img, const int* grp_npig, const int* weights, int max_weight, int K,
                               int A, int G, int sumG, int B, int I, int* npig_b, int* has_e_b, void* stream);
int omni_eval_bootstrap(const int* order, const int* cat_off, const int* rank, const int* dt_match, const unsigned char* dt_ignore,
                        const int* det_img, const int* weights, int max_weight, const int* npig_b, const int* has_e_b,
                        const double* rec_thrs, const int* max_dets, int K, int A, int M, int T, int R, int sumD, int B, int I,
                        double* ap, double* ar, void* stream);

/* The error decomposition of `Omni3Deval.errors` (csrc/eval_errors.hip): which mistake every false positive and every unfound ground
 * truth is, after TIDE (Bolya et al., ECCV 2020).  The reference has no counterpart and no call site.  Rows are ragged by IMAGE:
 * detections of image i are rows dt_off[i] .. dt_off[i + 1] - 1, ground truths gt_off[i] .. gt_off[i + 1] - 1 (both (I + 1) int32,
 * starting at 0, non-decreasing, ending at sumD / sumG; not checked here), over all categories; sim holds image i's (D_i, G_i) row-major
 * similarity matrix at sim_off[i] ((I + 1) int64).  Per detection: dt_cat, dt_matched (dt_match >= 0), dt_ignore, dt_score; per ground
 * truth: gt_cat, gt_matched, gt_ignore (`_ignore` at the analysed range; such a row is no candidate): the tables of omni_eval_match at
 * one (range, threshold).  0 < t_bg < t_fg.  Out, per detection: type (sumD) int8 = 0 true positive (matched, not ignored), 1 ignored,
 * and for every other one, with s_free / s_used / s_other = its largest similarity to an unmatched / a matched candidate of its own
 * category / a candidate of another category (-inf for an empty set, the later row among equal values), in this order: 3 Loc (s_free
 * >= t_bg), 2 Cls (s_other >= t_fg), 5 Dupe (s_used >= t_fg), 6 Bkg (all three < t_bg), 4 Both (the rest); similarities are compared
 * with the thresholds as doubles.  attr (sumD) = the global row of the arg-max of the deciding set for Loc / Cls / Dupe, -1 otherwise;
 * smax (sumD,3) = (s_free, s_used, s_other); win_loc (sumD) = 1 for the Loc detection with the highest score among those attributed to
 * the same ground truth (the lower row among equal scores); win_cls (sumD) = the same among the Cls detections, and only when that
 * ground truth is unmatched.  Per ground truth: gt_missed (sumG) = 1 for an unmatched candidate that is the attributed ground truth of
 * no Loc or Cls detection.  One 256-thread workgroup per image, one detection per thread; integer LDS atomics only: two runs give the
 * same bits.  max_gt = the largest G_i: above 1024 (the LDS capacity), as on negative sizes, thresholds out of order or a missing array,
 * OMNI_ERR_ARG before any launch; nothing is truncated.  I == 0 launches nothing; images without detections or ground truths are valid. */
int omni_eval_error_types(const float* sim, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_cat,
                          const unsigned char* dt_matched, const unsigned char* dt_ignore, const double* dt_score, const int* gt_cat,
                          const unsigned char* gt_matched, const unsigned char* gt_ignore, double t_fg, double t_bg, int I, int sumD,
                          int sumG, int max_gt, signed char* type, int* attr, float* smax, unsigned char* win_loc,
                          unsigned char* win_cls, unsigned char* gt_missed, void* stream);

/* Drawing predicted cuboids (csrc/render.hip).  The reference renders them with pytorch3d's mesh rasteriser and paints the edges
 * with OpenCV; here every pixel casts its ray (through the pixel centre (x + 0.5, y + 0.5)) against the boxes themselves.
 *
 * omni_cuboid_depth -- `render_depth_map` / `estimate_visibility` (cubercnn/util/math_util.py:707-743; the rasteriser call
 * `renderer(mesh)` at :719 and the per-box silhouette sums at :738-739).  box3d (N,6) [X,Y,Z,W,H,L] camera space, R (N,9), K (9),
 * vertices / faces as get_cuboid_verts_faces; zplane > 0.  Per pixel: depth (H,W) camera z of the first surface point at depth >=
 * zplane (the exit face when the entry lies in front of the plane), +inf without a hit; index (H,W) the box, -1 without a hit,
 * equal depths go to the lower index; face (H,W) 0..5 = front, right, left, back, top, bottom (the face pairs of the triangle list).
 * Per box: area (N) pixels whose ray hits the box at all at depth >= zplane, visible (N) pixels where it is the nearest hit (both
 * zeroed here; integer atomics only: two runs are bit-identical). */
int omni_cuboid_depth(const float* box3d, const float* R, const float* K, int N, int H, int W, float zplane, float* depth,
                      int* index, int* face, int* area, int* visible, void* stream);
/* The shaded overlay of `draw_scene_view` (cubercnn/vis/vis.py:278-282 and :382-384: `renderer(meshes_scene)` with PointLights at
 * the origin + SoftPhongShader, math_util.py:823-826): for every pixel with index >= 0, image (3,H,W) uint8 = round(shaded * blend_weight
 * + image * (1 - blend_weight)), shaded = 255 * color[index] (N,3 in [0,1]) * (0.5 + 0.3 * max(0, n . l)): n the outward normal of
 * `face`, turned to the viewer when the exit face was hit, l the unit vector from the hit point to the light at the camera origin.
 * No specular term.  Pixels without a hit are not touched.  0 <= blend_weight <= 1. */
int omni_scene_compose(const int* index, const int* face, const float* R, const float* K, const float* color, int N, int H, int W,
                       float blend_weight, unsigned char* image, void* stream);
/* `cv2.line` of draw_3d_box_from_verts (vis.py:622-626) as a gather: seg (S,8) = [x0, y0, x1, y1, thickness, c0, c1, c2]; every pixel
 * of image (3,H,W) uint8 whose centre lies within thickness / 2 of a segment takes (c0, c1, c2) (planes 0..2, rounded, clamped to
 * 0..255) of the LAST such segment of the list; the others are not touched.  A segment of length zero draws a disc. */
int omni_draw_segments(const float* seg, int S, unsigned char* image, int H, int W, void* stream);
/* Area fills blended in list order (csrc/shapes.hip): `draw_transparent_polygon`, `cv2.circle` and `draw_transparent_square`
 * (vis.py:540-568, 684-703) as a gather.  shape (S,13) = [kind, x0, y0, x1, y1, x2, y2, x3, y3, blend, c0, c1, c2] on image
 * (3,H,W) uint8.  kind 0: the quadrilateral (x0,y0) .. (x3,y3), vertices in order; a pixel is inside by the even-odd rule at its
 * centre (x + 0.5, y + 0.5), so a folded quadrilateral leaves its doubly covered part out.  kind 1: the ring with centre (x0,y0),
 * outer radius x1 and inner radius y1 (0: a disc): inside when inner <= distance of the centre <= outer.  Every pixel walks the
 * list in order; a covering shape replaces each plane's value v by floor(v * blend + (1 - blend) * c), evaluated in double with one
 * rounding per operation (numpy's float64 expression stored into uint8; clamped to 0..255), later shapes on the result of earlier
 * ones.  Pixels no shape covers are not touched.  A row with a value that is not finite, another kind or a negative outer radius
 * covers nothing; S = 0 launches nothing.  No atomics: two runs give the same bits. */
int omni_fill_shapes(const float* shape, int S, unsigned char* image, int H, int W, void* stream);
/* The ground plane of the novel view (vis.py:389-490; csrc/shapes.hip), per pixel and without a point mesh.  image (3,H,W) uint8;
 * index (H,W) int32 or NULL: pixels with index >= 0 (omni_cuboid_depth: a box is seen there) keep their bytes, every other pixel
 * is written.  K (9); the scene reaches view space by the rigid motion p' = A p + t (A (9) a rotation, t (3)); the plane is y = y0
 * in scene coordinates; near > 0; thickness >= 0 in pixels; colours as 0xRRGGBB (plane 0 takes RR).  The lines are the reference's:
 * X = k for k = x_start .. x_end - 2 over Z in [z_start, z_end - 1], and Z = k for k = z_start .. z_end - 2 over X in [x_start,
 * x_end - 1]; none when x_end - x_start < 2 or z_end - z_start < 2.  The ray through the pixel centre meets the plane at P = (X,
 * y0, Z).  The pixel takes bg_rgb when the ray does not meet the plane in front of the camera (nothing is drawn above the
 * horizon), when the view depth of P is below `near`, or when P lies outside the two spans; otherwise it takes line_rgb iff its
 * centre is within thickness / 2 pixels of the image of a drawn line next to P (k = floor and floor + 1 of X and of Z), bg_rgb if
 * not.  So a line ends square at the bounds and at `near` (the reference clamps depth to 0.25 and projects the clamped point,
 * which bends the line) and its end points are not truncated to integers.  |bounds| <= 2^24. */
int omni_ground_grid(unsigned char* image, const int* index, const float* K, const float* A, const float* t, float y0, int x_start,
                     int x_end, int z_start, int z_end, float near, float thickness, int bg_rgb, int line_rgb, int H, int W,
                     void* stream);

/* The 3D error report of `visualize_from_instances` (cubercnn/vis/vis.py:95-171, csrc/vis_errors.hip) for a whole dataset in one
 * call.  Rows are ragged by image: detections of image i are rows dt_off[i] .. dt_off[i + 1] - 1, ground truths gt_off[i] ..
 * gt_off[i + 1] - 1 (both (I + 1) int32, non-decreasing, ending at D / G; not checked here).
 *   detections   dt_box (D,4) XYWH, dt_cat (D) int32, dt_c2d (D,2) projected centre, dt_z (D), dt_dims (D,3) [w,h,l], dt_pose (D,9)
 *   ground truth gt_box (G,4) XYWH, gt_cat (G) int32, gt_center (G,3) camera space, gt_dims (G,3), gt_pose (G,9)
 *   K (I,9)      the intrinsics of every image, row-major
 * A detection is matched to the ground truth of its image and category with the largest 2D IoU (plain XYXY intersection over union,
 * no +1; 0 where the union is not positive; the lowest row among equal IoUs), valid at IoU >= 0.5.  Out:
 *   match (D) int32   global ground-truth row or -1
 *   err (D,7)         [xy, z, w, h, l, dim, ry] of the matched pair, NaN where match < 0: xy = |dt_c2d - (K gt_center / gt_center.z)[:2]|,
 *                     z = |dt_z - gt_center.z|, w / h / l = |differences of the dimensions|, dim = their Euclidean norm, ry = pi / 2 -
 *                     (trace(R_dt R_gt^T) - 1) / 2 (pytorch3d `so3_relative_angle(..., cos_bound=1)`), NaN and not counted when the trace
 *                     lies outside [-1 - 1e-4, 3 + 1e-4] (pytorch3d raises there and the reference skips the pair for ry)
 *   sums (7) double   the columns of err over the matched pairs (ry: over the pairs with a valid ry)
 *   counts (2) int64  matched pairs, matched pairs with a valid ry
 * workspace: I * 9 doubles (one row of partial sums per image, added in image order by a second launch: no floating-point atomics,
 * two runs give the same bits).  I = 0 (then D = G = 0) writes zero sums and counts. */
int omni_match_errors(const float* dt_box, const int* dt_cat, const float* dt_c2d, const float* dt_z, const float* dt_dims,
                      const float* dt_pose, const int* dt_off, const float* gt_box, const int* gt_cat, const float* gt_center,
                      const float* gt_dims, const float* gt_pose, const int* gt_off, const float* K, int I, int D, int G, int* match,
                      float* err, double* sums, long long* counts, double* workspace, void* stream);

/* The selection behind the training-time drawings of `RCNN3D.visualize_training` (csrc/train_vis.hip), for the training-mode rows of a
 * whole batch in one launch.  It stands for predict_boxes_for_gt_classes (cubercnn/modeling/roi_heads/roi_heads.py:276-281),
 * scores = exp(-uncertainty of the GT class) (:782-805) and `batched_nms(pred_boxes, scores, zeros, test_nms_thresh)[:20]`
 * (cubercnn/modeling/meta_arch/rcnn3d.py:207-214).
 *   pred (B*S, ldp)   box-head output [K+1 logits | 4K deltas]; head (B*Fc, ldh) cube-head output, uncert_off = column of its
 *                     uncertainty block ((5 + bins + Pn) * K), or -1 when USE_CONFIDENCE is 0: every score is then 1 and the rows keep
 *                     their order (the reference's score is, by accident of `cube_3D_i[:, -1]`, the v coordinate there)
 *   rois (B,Fc,4), cls (B,Fc) int32, nfg (B) int32: the cube prefix and the foreground count the sampler writes.  Image b uses pred
 *                     rows b*S + j and head rows b*Fc + j for j < nfg[b] (clamped to [0, min(Fc, S)])
 *   wx..wh, scale_clamp  Box2BoxTransform weights and clamp, as omni_box_decode_gt_class (the same device function, unclipped)
 * Per image: rows in descending score (ties to the lower row), greedy NMS -- j is suppressed after a kept i when
 * inter / (area_i + area_j - inter) > iou_thr in float32 (torchvision box_iou) -- until max_keep rows are kept.  A row whose box or
 * score is not finite, or whose class lies outside [0, K), is never kept and never suppresses.  Out:
 *   keep_row (B,max_keep) int32 the kept rows j in that order, -1 beyond keep_count (B) int32; keep_box (B,max_keep,4) and keep_score
 *   (B,max_keep), zero beyond the count.
 * One 256-thread workgroup per image, no atomics, two runs give the same bits.  Fc > 1024 (the LDS capacity) returns OMNI_ERR_ARG. */
int omni_train_vis_pick(const float* pred, int ldp, const float* head, int ldh, int uncert_off, const float* rois, const int* cls,
                        const int* nfg, int B, int S, int Fc, int K, float wx, float wy, float ww, float wh, float scale_clamp,
                        float iou_thr, int max_keep, int* keep_row, int* keep_count, float* keep_box, float* keep_score, void* stream);

/* Deriving the box fields of Omni3D annotations (csrc/annotate.hip) for a whole dataset in two calls.  Rows are ragged by image as
 * above: the boxes of image i are rows box_off[i] .. box_off[i + 1] - 1 (box_off (I + 1) int32, starting at 0, non-decreasing, ending
 * at N; not checked here).  box3d (N,6) [X,Y,Z,W,H,L] camera space, R (N,9), K (I,9) row-major, size (I,2) int32 [W, H].
 *
 * omni_box_annotate -- `get_cuboid_verts` (cubercnn/util/math_util.py:221-259), `convert_3d_box_to_2d` (:498-577, the projection at
 * :537, the behind test at :540-541, the corner substitution at :543-555, the box at :557-570) and `estimate_truncation` (:745-758)
 * for all N boxes, one thread per box.  Out:
 *   verts3d (N,8,3)       the vertices R v + centre in the order of get_cuboid_verts_faces (`bbox3D_cam`)
 *   verts2d (N,8,3)       [u, v, z] = [(K p).x / (K p).z, (K p).y / (K p).z, (K p).z] of every vertex p, before any substitution
 *   behind, fully_behind  (N) uint8: any / all of the vertices have z <= min_z (the reference's default min_z is 0.20)
 *   proj (N,4) XYXY       min and max of the eight points, where a vertex with z <= min_z is replaced by the image corner that the
 *                         signs of its camera-space x and y select (0 or W - 1, 0 or H - 1); the signs are compared strictly, so such a
 *                         vertex with x or y exactly 0 keeps its own projection, as in the reference.  A NaN stays (torch.min / max).
 *   truncation (N) double 1 when fully_behind, otherwise 1 - area(proj ^ [0, 0, W - 1, H - 1]) / area(proj), evaluated in float64 from
 *                         the float32 proj (the reference: numpy on the .tolist() values); NaN for a proj of zero area (0 / 0)
 *   trunc (N,4) XYXY      `bbox2D_trunc`, for which the reference has no code (only its annotation files carry the field).  Defined
 *                         here: proj intersected with [0, W - 1] x [0, H - 1]; [-1, -1, -1, -1] when the box is fully_behind or the
 *                         intersection has no area (x2 <= x1 or y2 <= y1, or proj holds a NaN).
 * No LDS, no atomics: two runs give the same bits.  N = 0 launches nothing. */
int omni_box_annotate(const float* box3d, const float* R, const int* box_off, const float* K, const int* size, int I, int N,
                      float min_z, float* verts3d, float* verts2d, float* proj, float* trunc, double* truncation,
                      unsigned char* behind, unsigned char* fully_behind, void* stream);
/* omni_visibility_ragged -- the counters of `estimate_visibility` (math_util.py:728-743: `silhouettes[annidx].sum()` at :738 and the
 * nearest-surface count at :739) for every box of every image: area (N) and visible (N) int32 are exactly the `area` / `visible` of
 * omni_cuboid_depth called once per image on the boxes of that image (same pixel centres, same zplane rule, equal depths to the
 * lower row; occlusion is judged among the boxes of the same image only), without any depth, index or face map.  One workgroup per
 * 16 x 16 tile of the concatenated tile list: tile_off (I + 1) int32 is the prefix sum of ceil(W / 16) * ceil(H / 16) over the
 * images (W, H > 0), tiles = tile_off[I].  Both outputs are zeroed here; integer atomics only: two runs give the same bits. */
int omni_visibility_ragged(const float* box3d, const float* R, const int* box_off, const float* K, const int* size,
                           const int* tile_off, int I, int N, int tiles, float zplane, int* area, int* visible, void* stream);

/* The KITTI object benchmark's protocol (csrc/eval_kitti.hip), for `cubercnn.evaluation.kitti.KittiEval`: AP|R40 and AP|R11 per
 * (class, difficulty, metric, overlap set).  The reference has no counterpart; the protocol is the project's reading of the devkit's
 * evaluate_object, stated in float64 by tests/exact_kitti.py.  A slot is s = ((c * Dn + d) * M + m) * O + o, S = C * Dn * M * O.
 * Rows are ragged by IMAGE: the detections of image i are rows dt_off[i] .. dt_off[i + 1] - 1 IN DESCENDING SCORE ORDER (stable), its
 * ground-truth rows gt_off[i] .. gt_off[i + 1] - 1 in input order, its DontCare regions dc_off[i] .. dc_off[i + 1] - 1 (all (I + 1)
 * int32 from 0, non-decreasing; not checked here).  sim (M, P) float32: for metric m, image i's (G_i, D_i) row-major matrix -- the
 * detections run fastest -- at sim[m * P + sim_off[i]] (sim_off (I) int64); dc_ov: image i's (R_i, D_i) matrix of (intersection /
 * area of the detection's 2D box) at dc_pair_off[i].  Per row: dt_code / gt_code int32 class codes, dt_height / gt_height /
 * gt_trunc / dt_score doubles, gt_occ int32.  Tables, all in device memory: cls_tab (C, ncodes) int32 = 0 where the code is class c
 * itself, 1 where it is a neighbour class of c, 2 where it is class c set aside by the caller (ground truths only: a detection of
 * class c has a code with 0), anything else (and every code outside [0, ncodes)) for the rest; diffs (Dn, 3)
 * doubles (min height, max occlusion, max truncation); min_ov (O, C) doubles, ALL >= 0 (the caller's to keep: pass 2 orders overlaps
 * by their bit patterns); dc_metric (M) int32, non-zero where DontCare regions absorb false positives.
 *   ground-truth flag: 0 (counted) the class itself with occ <= max occlusion, trunc <= max truncation, height >= min height; 1
 *   (neutral) the class itself otherwise -- set aside or not --, and every neighbour; -1 the rest, a row set aside that those three
 *   bounds would count included.  detection flag: -1 another class, 1 height < min height,
 *   else 0.  An overlap qualifies when (double)sim > min_ov, strictly.
 * omni_kitti_match_tp -- pass 1, one 64-lane wave per (image, slot): every ground truth with flag >= 0, in order, takes the unassigned
 *   detection of its class with a qualifying overlap and the largest score (the earliest among equal scores).  tp_score (S, sumG) =
 *   that score when both flags are 0, -inf otherwise (every element is written); n_gt (S), ZEROED BY THE CALLER, += the flag-0 rows.
 * omni_kitti_thresholds -- one workgroup per slot: with v = the finite entries of the slot's tp_score in descending order, i runs over
 *   them with l = (i + 1) / n_gt, r = (i + 2) / n_gt (l for the last), and v[i] is emitted unless it is not the last and r - cur <
 *   cur - l; cur starts at 0 and grows by 1 / (npts - 1) per emission; at most npts are emitted.  thresholds (S, npts) = the emitted
 *   scores, bit for bit, 0 beyond K (S) = their number.  No host round trip: pass 2 reads K on the device.
 * omni_kitti_match_counts -- pass 2, one wave per (image, slot, k), idle for k >= K[s]: detections scoring below thresholds[s][k] do
 *   not exist.  Every ground truth with flag >= 0, in order, takes the unassigned flag-0 detection with the largest qualifying overlap
 *   (the earliest among equals), or without one the earliest qualifying flag-1 detection.  Nothing taken and flag 0: fn; taken and both
 *   flags 0: tp.  fp = the unassigned flag-0 detections, less -- where dc_metric[m] -- those with dc_ov > min_ov on any region.
 *   counts (S, npts, 3) int32 (tp, fp, fn), ZEROED BY THE CALLER, integer atomics only: two runs give the same bits.
 * omni_kitti_finalize -- precision (S, npts) = tp / (tp + fp) and recall = tp / (tp + fn) for k < K (0 for an empty denominator and
 *   for k >= K), precision replaced by its running maximum from the right; ap (S, 2) = 100 x the mean of precision[1 .. npts - 1]
 *   (R40 for npts = 41) and 100 x the mean of precision[0, 4, 8, ...] (R11), summed in ascending k, all in double.
 * OMNI_ERR_ARG before any launch: a negative size, max_dt or max_gt (the caller's largest per-image counts) above 1024, npts outside
 * [2, 64], I x S (omni_kitti_match_tp) or I x S x npts (omni_kitti_match_counts) >= 2^26: one workgroup per problem.  I == 0 or S == 0
 * launches nothing and returns OMNI_OK. */
int omni_kitti_match_tp(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                        const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                        const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov, int I, int C,
                        int Dn, int M, int O, int sumD, int sumG, int max_dt, int max_gt, double* tp_score, int* n_gt, void* stream);
int omni_kitti_thresholds(const double* tp_score, const int* n_gt, int S, int sumG, int npts, double* thresholds, int* K, void* stream);
int omni_kitti_match_counts(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                            const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                            const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov,
                            const float* dc_ov, const long long* dc_pair_off, const int* dc_off, const int* dc_metric,
                            const double* thresholds, const int* K, int npts, int I, int C, int Dn, int M, int O, int sumD, int sumG,
                            int max_dt, int max_gt, int* counts, void* stream);
int omni_kitti_finalize(const int* counts, const int* K, int S, int npts, double* precision, double* recall, double* ap, void* stream);

/* AOS, the benchmark's average orientation similarity (csrc/eval_kitti.hip; the project's reading of the devkit's compute_aos path,
 * written from memory; float64 statement: tests/exact_kitti_aos.py).
 * omni_kitti_match_counts_aos -- omni_kitti_match_counts (counts: the same bits) and, for every true positive (the condition under
 *   which tp is incremented) of a slot whose metric has aos_metric[m] != 0, q = (1 + cos(gt_alpha[row] - dt_alpha[detection])) / 2 in
 *   double, 0 when either alpha is not finite (NaN: no heading).  sim_sum (S, npts) 64-bit integers, ZEROED BY THE CALLER, +=
 *   llrint(q * 2^40): fixed point, integer atomics (one per wave), so two runs give the same bits.  dt_alpha (sumD), gt_alpha (sumG)
 *   float64, aos_metric (M) int32.  OMNI_ERR_ARG also for sumG >= 2^23, the bound under which the sum cannot overflow.
 * omni_kitti_finalize_aos -- aos (S, npts) = sim_sum * 2^-40 / (tp + fp) for k < K (0 for an empty denominator and for k >= K),
 *   replaced by its running maximum from the right over k < K; aos_ap (S, 2) = 100 x the mean of aos[1 .. npts - 1] and of
 *   aos[0, 4, 8, ...], in the order of omni_kitti_finalize.  A slot of a metric with aos_metric[m] == 0: NaN in both. */
int omni_kitti_match_counts_aos(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                                const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                                const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov,
                                const float* dc_ov, const long long* dc_pair_off, const int* dc_off, const int* dc_metric,
                                const double* thresholds, const int* K, int npts, int I, int C, int Dn, int M, int O, int sumD, int sumG,
                                int max_dt, int max_gt, const double* dt_alpha, const double* gt_alpha, const int* aos_metric, int* counts,
                                long long* sim_sum, void* stream);
int omni_kitti_finalize_aos(const int* counts, const long long* sim_sum, const int* K, const int* aos_metric, int S, int M, int O, int npts,
                            double* aos, double* aos_ap, void* stream);

/* Cuboid corners -> the KITTI object benchmark's box parameters (csrc/kitti_params.hip), one thread per box, double arithmetic on the
 * float32 corners.  corners (n, 8, 3) in the corner order of omni_cuboid_corners: l = |v1 - v0|, h = |v3 - v0|, w = |v4 - v0|, c = the
 * mean of the eight corners.  u = up normalised, a = camera x less its part along u, normalised, b = u x a (up (0, -1, 0): a = x,
 * b = z).  out (n, 9) float64: h, w, l, (x, y, z) = c - (h / 2) u (the centre of the bottom face), rotation_y = atan2(-e.b, e.a) with
 * e = v1 - v0 (0 for a heading without a ground-plane component), alpha = rotation_y - atan2(c.a, c.b) wrapped into (-pi, pi], valid.
 * valid = 1 when all 24 inputs are finite and l, h, w > 0; otherwise 0 and the other eight are NaN.  OMNI_ERR_ARG: n < 0, an up vector
 * of zero or non-finite length or parallel to camera x. */
int omni_kitti_box_params(const float* corners, int n, double up_x, double up_y, double up_z, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OMNI3D_HIP_H */
