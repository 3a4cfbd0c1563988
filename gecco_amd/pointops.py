"""Point-cloud operators on the HIP device: farthest-point sampling (csrc/fps.hip, gecco_fps_f32), k-nearest-neighbour search
(csrc/knn.hip, gecco_knn_f32) with the statistical outlier filter built on it, surface normals with curvature from the neighbour
lists (csrc/normals.hip, gecco_normals_f32), voxel-grid downsampling with attribute pooling (csrc/voxel.hip,
gecco_voxel_downsample_f32), rigid ICP registration, point-to-point and point-to-plane (csrc/icp.hip, gecco_icp_f32), FPFH
descriptors with nearest-neighbour matching in feature space (csrc/fpfh.hip, gecco_fpfh_f32, gecco_feature_nn_f32), and RANSAC
registration from correspondences (csrc/ransac.hip, gecco_ransac_f32), RANSAC plane segmentation (csrc/plane.hip,
gecco_plane_ransac_f32), DBSCAN clustering (csrc/dbscan.hip, gecco_dbscan_f32) and fixed-radius neighbour search (csrc/radius.hip,
gecco_radius_count_f32, gecco_radius_search_f32) with the radius outlier filter built on it and a uniform-grid index for large clouds
(csrc/grid.hip, gecco_grid_build_f32), and ISS keypoint detection on that index (csrc/iss.hip, gecco_iss_keypoints_f32).

The reference reduces a dense cloud to a fixed size by random permutation (gecco-jax data/torch_shapenet.py:20-21, data/taskonomy.py:84),
which keeps density clumps and loses thin structure.  `farthest_point_sample` is the well-spread cut: from a start point, each next point
is the one farthest from those chosen so far.

Definition (the one include/gecco_hip.h states and tests/_fps_ref.py restates in numpy float32).  With d_i = +inf and s_0 = start:
    for t = 0 .. k-1:  idx[t] = s_t;  sel2[t] = d_{s_t};  d_i = min(d_i, dist2(p_i, p_{s_t}));  s_{t+1} = argmax_i d_i
where dist2(a, b) = (dx*dx + dy*dy) + dz*dz on the coordinate differences, every operation rounded to fp32 without FMA contraction, and
the argmax takes the LOWEST index among equal maxima.  Near-ties are closer than one rounding, so the roundings are the definition: the
indices are the same bits run to run, in any batch position and in both kernel forms (a maximum of integer keys, no float atomics).
Duplicate points: once every remaining distance is 0 the lowest index wins again and indices repeat (ten identical points, start 3,
k = 4: [3, 0, 0, 0]).  NaN coordinates: the selection in that cloud is unspecified, its indices stay in [0, N), other clouds are untouched.

Two forms.  "resident": one workgroup per cloud and one launch for the whole batch and all k steps, coordinates and running distances in
registers; N <= FPS_RESIDENT_MAX_POINTS (8192: every evaluation and training shape).  "streaming": any N, the running distances in a
workspace, several workgroups per cloud and ONE launch per selected point (no workgroup ever waits on another, so the chain cannot hang);
the 100 000-point output of `Diffusion.upsample` is its case.  form=None takes the resident form when N fits and the streaming form above.

k nearest neighbours (`knn`, `knn_gather`, `statistical_outlier_mask`).  The reference has no neighbourhood query; the route without
this module is `metrics.distance_matrix` + `torch.topk`, an M x N matrix (40 GB for a 100 000-point cloud against itself) of
aa + bb - 2ab distances whose cancellation noise reorders near neighbours.  Definition (include/gecco_hip.h; tests/_knn_ref.py restates
it in numpy float32).  For queries q_i (i < M) and reference points p_j (j < N) of the same batch element,
    dist2(q, p) = (dx*dx + dy*dy) + dz*dz
on the coordinate differences, every operation rounded to fp32 without FMA contraction (the spelling of the sampling above).  A NaN dist2
is replaced by +inf.  The pairs of query i are ordered by (dist2, j) ascending, equal distances going to the LOWEST index, and the result is
the first k pairs in that order: idx[i, t], and d2[i, t] non-decreasing in t.  Self mode (the query cloud is the reference cloud and
exclude_self is set) skips the pair j == i by index, not by distance, so exact duplicates of a point remain candidates at distance 0.
On the 6 x 6 x 6 integer grid (meshgrid(indexing="ij").reshape(-1, 3)) in self mode with k = 7, query 0 gets [1, 6, 36, 7, 37, 42, 43]
with d2 = [1, 1, 1, 2, 2, 2, 3] and query 215 gets [179, 209, 214, 173, 178, 208, 172]; without self exclusion, k = 4, query 0 gets
[0, 1, 6, 36].  Ten identical points, query 3, k = 4: self mode gives [0, 1, 2, 4], all at distance 0; without exclusion [0, 1, 2, 3].
Indices are always in [0, N).  A NaN coordinate affects only the rows and candidates it touches: a NaN reference point is chosen only
after every finite one, a NaN query returns [0, 1, ..., k-1] (in self mode the first k indices other than its own) with dist = +inf, other
batch elements are untouched.  The outputs are the same bits run to run, in any batch position and in both kernel forms: the order is that
of one monotone integer key per pair (dist2's bits above j), so there are no float atomics and the merge of the split form is exact.
Two forms.  "direct": one launch, one thread per query, the reference cloud streamed through LDS.  "split": few queries against many
points (M = 2048 conditioning points against the upsampler's N = 100 000): the reference cloud is cut into slices of KNN_SPLIT_SLICE
points, one launch finds each slice's k best, a second merges them.  form=None takes the split form when the direct grid would leave
compute units idle and N spans more than one slice.  1 <= k <= KNN_MAX_K.

Normals and curvature (`estimate_normals`).  What PCL and Open3D compute directly after the neighbour search: the PCA normal of each
point's k-neighbourhood and its "surface variation".  The route without it is `knn_gather` (a (B, M, k, 3) tensor), a mean, an einsum
and `torch.linalg.eigh` on B * M little 3 x 3 matrices.  Definition (include/gecco_hip.h; tests/_normals_ref.py restates it in numpy
float32).  For query i, searched with the point itself among the candidates (a point belongs to its own neighbourhood):
    neighbourhood  the reference points idx[i, t] with dist2[i, t] <= fp32(radius * radius), or all k of them without a radius; their
                   number m is `count` (the hybrid search of Open3D)
    covariance     mu = sum p / m;  C = sum (p - mu)(p - mu)^T / m: two passes, centred, in fp32 (not the raw moments E[pp^T] - mu mu^T,
                   which lose every digit on a cloud far from the origin)
    eigenpairs     of C, lambda0 <= lambda1 <= lambda2, by 4 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) on C / trace(C): a fixed
                   count.  A rotation whose parameter (a_qq - a_pp) / (2 a_pq) is not finite is skipped, one whose square would
                   overflow takes t = 1 / (2 theta); negative roundings of an eigenvalue are clamped to 0
    normal         the unit eigenvector of lambda0;  curvature = lambda0 / (lambda0 + lambda1 + lambda2)
    invalid rows   m < 3, a non-finite coordinate in the query or a counted neighbour, trace(C) not a positive finite number (0: all
                   counted points identical), an index outside [0, N): normal = (0, 0, 1) as in Open3D, eigenvalues = 0,
                   curvature = 0, count still m.  A collinear neighbourhood is valid: some unit vector of the null space
    sign           valid rows only.  With a viewpoint v: n . (v - q_i) >= 0.  Without: the component of largest magnitude is positive,
                   the lowest axis among equal magnitudes
One query's result depends on its own neighbour list and the points it names, nothing else: no atomics, the same bits run to run, in
any batch position and through either form of the search.  Against float64 `eigh` of the float64 covariance of the same fp32
coordinates, |C n - lambda0 n| and every eigenvalue stay within 32 * 2^-24 * trace(C).

Voxel-grid downsampling (`voxel_downsample`, `voxel_pool`).  The filter PCL and Open3D put before all of the above: one point per
occupied cell of a regular grid, at the centroid of the cell's points; O(N) and five launches whatever the output size, where the
streaming farthest-point form needs one launch per kept point.  The route without it is `torch.floor` -> `torch.unique(dim=0,
return_inverse=True)` (a sort over N rows and a synchronisation) -> `index_add` (float atomics: not reproducible).  Definition
(include/gecco_hip.h; tests/_voxel_ref.py restates it in numpy).  With the voxel size s > 0 rounded to fp32, an origin o of three fp32
values per cloud (default 0: the grid is anchored at the world origin and needs no pass over the cloud) and inv = fp32(1 / s):
    cell       per axis t = fp32(p - o), u = fp32(t * inv), c = floor(u).  A point is DROPPED when any u is not finite or any c is
               outside [-2^20, 2^20): it belongs to no voxel and its `inverse` is -1
    key        (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), 63 bits
    voxels     the distinct keys of a cloud's kept points, numbered in order of FIRST OCCURRENCE (voxel v before voxel w when the
               lowest point index in v is below the lowest in w); first[v] = that lowest index, count[v] = the number of points
               in v, inverse[i] = the voxel of point i, n_voxels = their number
    centroid   frac = fp32(u - c) per axis (it can round to 1.0 for a tiny negative u: part of the definition), q = (uint64)
               trunc(frac * 2^32), S[v] = the exact integer sum of q over the voxel, centroid = fp32(double(o) + (double(c) +
               double(S) / (double(count) * 2^32)) * double(s)), every fp64 operation rounded and none contracted
    max_voxels given: every output holds max_voxels rows per cloud, rows at or after n_voxels are zero with count = 0 and first = -1,
               points of voxels numbered max_voxels or higher get inverse = -1, and n_voxels is reported unclamped
s = 1, o = 0, points (.5,.5,.5), (.6,.5,.5), (1.5,.5,.5), (.4,.4,.4), (-.25,.5,.5), (NaN,0,0): inverse = [0, 0, 1, 0, 2, -1], first =
[0, 2, 4], count = [3, 1, 1], centroids (0.5, 0.46666667, 0.46666667), (1.5, .5, .5), (-.25, .5, .5).  Integer sums do not depend on
arrival order and the numbering is a scan over the point index: the outputs are the same bits run to run, in any batch position and
for any launch geometry; no float atomics, no sort, no thread waits on another.

ICP registration (`icp`, `transform_points`).  The consumer PCL and Open3D put behind all of the above: the rigid transformation that
maps a source cloud onto a target cloud (a generated cloud onto a scan, a cloud before and after `Diffusion.upsample`).  The route
without it is `knn(k=1)` -> `knn_gather` -> `torch.linalg.svd` in a Python loop with one host synchronisation per iteration, and no
point-to-plane form although `estimate_normals` produces the normals it needs.  The definition follows Open3D's `registration_icp`
(include/gecco_hip.h; tests/_icp_ref.py restates it in numpy).  Each cloud of the batch is independent; its state T is a 4 x 4 fp64
matrix starting at `init`; r2 = fp32(r * r) with the product taken in double; the anchor is c = double(target[0]).  Pass i = 0, 1, ...:
    1 transform  Tf = fp32(T);  p'_m = ((Tf[a][0] x + Tf[a][1] y) + Tf[a][2] z) + Tf[a][3] per axis a, every operation rounded to fp32
                 and none contracted
    2 match      (d2_m, j_m) = the first pair of knn(p', target, k=1): the search's own dist2 spelling, NaN -> +inf, equal distances to
                 the LOWEST index.  Pair m is an inlier when d2_m <= r2 (a NaN source point has d2 = +inf and is never one); in the
                 plane method the three components of n_{j_m} must be finite as well
    3 measure    n = the number of inliers;  fitness_i = n / M;  rmse_i = sqrt(sum d2 / n), the sum in fp64, 0 when n = 0
    4 stop       at the first that holds.  status 3: `init` has a non-finite entry (pass 0 only).  status 0: i >= 1 and |fitness_i -
                 fitness_{i-1}| < relative_fitness and |rmse_i - rmse_{i-1}| < relative_rmse (absolute differences, as in Open3D
                 despite the names).  status 1: i == max_iterations.  status 2: n < 3 (point) / n < 6 (plane) or a singular system.
                 T is left as it is; the outputs are this pass's fitness, rmse and correspondences (j_m for inliers, -1 otherwise)
                 and iterations = i
    5 update     T <- dT * double(Tf).  point_to_point: for the inlier pairs P = double(p'), Q = double(q) the centroids and the
                 cross-covariance from moments about c in fp64, Horn's 4 x 4 symmetric matrix, its largest eigenvector by 8 cyclic
                 Jacobi sweeps in fp64 (a fixed count; the rotation guarded as in the normals), the quaternion normalised with
                 w >= 0, R from it and t = mu_q - R mu_p; a collinear inlier set is valid, it yields some rotation.  point_to_plane:
                 res_m = (p'_m - q_m) . n_m, J_m = [(p'_m - c) x n_m, n_m], A = sum J^T J and g = sum J res in fp64, A x = -g by LDL^T
                 without pivoting (singular: a pivot non-finite or <= 2^-36 max diag(A)), dT = Trans(c) [Rz(x2) Ry(x1) Rx(x0) | x3..5]
                 Trans(-c); normals are used as given
max_iterations = 0 is Open3D's `evaluate_registration`: one matching pass under `init`, no change of T, status 1.  A NaN target point
is never matched while a finite one exists; neither disturbs another cloud.  Source (0,0,0), (1,0,0), (0,1,0), (0,0,1) against the same
four points moved by (0.25, 0, 0), r = 1, point_to_point: pass 0 pairs every point with its moved self (d2 = 0.0625, fitness 1, rmse
0.25) and finds the translation; pass 1 measures rmse 0 and updates by the identity; pass 2 sees no change and stops: status 0,
iterations 2, T = the translation by (0.25, 0, 0).  Two launches per pass, 2 * (max_iterations + 1) for a call whatever the data: no
atomics, no workgroup waits on another and no host synchronisation, so a call can be captured in a hipGraph; a stopped cloud costs
two empty launches per remaining pass.  The outputs are the same bits run to run, in any batch position and in both forms of the
match ("direct" / "split", the forms and the auto rule of `knn`).

FPFH descriptors and feature matching (`fpfh`, `match_features`).  `icp` converges only from a good `init`; what produces one is a
global registration on local descriptors (the pose estimator is `ransac_registration`, below).  `fpfh` is Fast Point Feature
Histograms (Rusu et al. 2009) in the form Open3D's
`compute_fpfh_feature` and PCL's `FPFHEstimation` compute: FPFH_BINS = 33 numbers per point from the neighbour list and the normals
the functions above already produce.  The route without it is `knn_gather`, about twenty torch ops with float atomics for the
histograms, and `torch.cdist` (an M x N matrix) for the matching.  Definition (include/gecco_hip.h; tests/_fpfh_ref.py restates it in
numpy).  For point i and neighbour j, in fp64 on the fp32 inputs, every operation rounded and none contracted into an FMA (bin edges
make the histogram discontinuous; in fp32 two evaluations disagree on a bin every few thousand pairs):
    1  P1, N1, P2, N2 = double(p_i, n_i, p_j, n_j);  dp = P2 - P1;  d = sqrt((dx dx + dy dy) + dz dz)
    2  d == 0: f = (0, 0, 0)
    3  a1 = ((N1x dpx + N1y dpy) + N1z dpz) / d;  a2 the same with N2
    4  |a1| < |a2|: swap N1 <-> N2, negate dp, f2 = -a2; otherwise f2 = a1 (Open3D's acos(|a1|) > acos(|a2|) without the acos)
    5  v = dp x N1;  vn = |v| in the spelling of d
    6  vn == 0: f = (0, 0, 0), all three components, as in Open3D
    7  v = v / vn;  w = N1 x v;  f1 = v . N2;  f0 = atan2(w . N2, N1 . N2)
    8  u0 = (11 (f0 + pi)) / (2 pi);  u1 = (11 (f1 + 1)) 0.5;  u2 = (11 (f2 + 1)) 0.5;  b_g = clamp(floor(u_g), 0, 10)
    9  the pair adds one count to each of the bins b0, 11 + b1, 22 + b2
Normals are used as given.  The list idx[i, 0 .. k) is that of `knn(points, points, k, exclude_self=False)`, the list
`estimate_normals` uses: one search serves both.  Entry t counts when 0 <= j < N; j != i, by index (an exact duplicate of the point
stays a neighbour and contributes the zero triple: bins 5, 16, 27); with a radius, dist2(p_i, p_j) <= fp32(radius^2), the distance
recomputed from the coordinates with the search's roundings; and all twelve numbers of p_i, n_i, p_j, n_j are finite.  m_i = the number
of counted entries (`count`).
    SPFH  spfh[i, b] = fp32((100.0 count_b) / m_i) in double, a zero row when m_i = 0: integer counts, one rounding; each of the three
          groups of a non-empty row sums to 100
    FPFH  over the entries of i's list in list order that were counted, have dist2 != 0 and m_j > 0: w_t = 1 / double(dist2_t),
          W = sum w_t, acc[b] = sum w_t double(spfh[j_t, b]);  fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0)).
          Open3D's per-group factor 100 / sum_group is 1 / W because every non-empty SPFH group sums to 100; written this way no
          cross-bin reduction order enters the definition.  The point's own SPFH is added unweighted, as in PCL and Open3D
Points (0,0,0), (1,0,0), (0,1,0), all normals (0,0,1), k = 3: every pair gives f = (0, 0, 0), u = 5.5; every SPFH row is 100 at bins
5, 16, 27 and every FPFH row 200 there, 0 elsewhere.  Points (0,0,0) with normal (0,0,1) and (1,0,0) with normal (0.6, 0, 0.8), k = 2:
from point 0 a1 = 0, a2 = 0.6, the swap happens, f2 = -0.6, u2 = 2.2, v = (0,1,0), f1 = 0, u1 = 5.5, f0 = atan2(0.6, 0.8), u0 = 6.63;
from point 1 no swap and the same triple: both SPFH rows are 100 at bins 6, 16, 24, both FPFH rows 200 there.
`match_features`: for a (B, M, C) and b (B, N, C), 1 <= C <= FEATURE_MAX_DIM, d2(i, j) = sum_c (a_ic - b_jc)^2 accumulated from 0 in
the order c = 0 .. C - 1, every operation rounded to fp32 and none contracted; a NaN d2 becomes +inf; the match of row i is the j of
the smallest (d2, j), the LOWEST index among equal distances (one monotone 64-bit key per pair, the spelling of `knn`); a query whose
every d2 is +inf gets j = 0 and d2 = +inf.  No M x N matrix is formed.  Mutual: corr[i] = j_i if the match of b[j_i] in a is i, else -1
(the reverse search plus a gather and a compare in torch).  The forms "direct" / "split" and the auto rule are those of `knn`.
No atomics and no thread waits on another: the same bits run to run, in any batch position, in both forms of either search and with
`idx` given or searched.  A non-finite point or normal changes the SPFH rows whose lists name it and the FPFH rows whose lists name it
or one of those rows, nothing else.

RANSAC registration from correspondences (`ransac_registration`).  The pose estimator between `match_features` and `icp`: Open3D's
`registration_ransac_based_on_correspondence` (the core of `registration_ransac_based_on_feature_matching`) with a fixed number of
hypotheses, so that `fpfh` -> `match_features` -> `ransac_registration` -> `icp` registers two clouds from any relative pose without
leaving the device.  The route without it is a Python loop of `torch.randint`, a batched `torch.linalg.svd` and an (H, K, 3) tensor
per chunk.  Definition (include/gecco_hip.h; tests/_ransac_ref.py restates it in numpy).  Per cloud, with r2 = fp32(r * r) as in `icp`:
    pairs   the source indices i in ascending order with 0 <= corr[i] < N (an index outside is never dereferenced) and all six
            coordinates of p_i and q_corr[i] finite; K of them (`n_pairs`); P_a, Q_a the a-th pair; c = double(Q_0)
    draw    for h = 0 .. H - 1, all mod 2^64:  mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
            z ^= z >> 31.  u_t = mix(seed + (3 h + t + 1) * 0x9E3779B97F4A7C15), t = 0, 1, 2;  draw_t = ((u_t >> 32) * (K - t)) >> 32;
            a0 = draw_0;  a1 = draw_1 + (draw_1 >= a0);  lo, hi = min, max(a0, a1);  a2 = draw_2; a2 += (a2 >= lo); a2 += (a2 >= hi):
            three distinct indices in [0, K) without a rejection loop, pure integer work
    checks  in this order, in fp64 on the fp32 coordinates, every operation rounded, none contracted, |d|^2 = (dx dx + dy dy) + dz dz,
            no division and no root:
            1  degenerate triangle, for X = P and then X = Q: e1 = X_a1 - X_a0, e2 = X_a2 - X_a0, n = e1 x e2; rejected (code 1) when
               |n|^2 <= 2^-20 (|e1|^2 |e2|^2), which also catches coincident points
            2  edge length (Open3D's CorrespondenceCheckerBasedOnEdgeLength), s2 = edge_similarity^2: every edge (a0, a1), (a1, a2),
               (a2, a0) needs |P_a - P_b|^2 >= s2 |Q_a - Q_b|^2 and |Q_a - Q_b|^2 >= s2 |P_a - P_b|^2 (code 2); 0 switches it off
            3  fit: Horn's quaternion on the three pairs from fp64 moments about double(Q_a0) summed in the order a0, a1, a2, by the
               routine of `icp`'s update; a non-finite T is code 4
            4  distance (Open3D's CorrespondenceCheckerBasedOnDistance): under Tf = fp32(T), with `icp`'s transform spelling and
               `knn`'s dist2 spelling, each of the three pairs needs d2 <= r2 (code 3)
            5  score over all K pairs in pair order: count = the number with d2 <= r2, sum = the fp64 sum of double(d2) over those,
               accumulated sequentially in pair order
            per hypothesis, with return_hypotheses: the triple, count (or -code), sum (or +inf).  K < 3: triple -1, count -1, sum +inf
    candidates  given, T = candidates[b, h] replaces the draw and checks 1 - 3, and check 4 is skipped; a non-finite entry is code 4;
            the triples are -1.  It scores poses of one's own (symmetric alternatives)
    select  the surviving hypothesis with count >= 3 that is best under (count descending, sum ascending, h ascending): a total order,
            so the shape of the reduction cannot change it
    refine  refine_passes times: the inliers of the current T among the K pairs, fp64 moments about c reduced in a fixed order, Horn,
            T <- dT * double(Tf).  A pass with fewer than 3 inliers or a non-finite dT leaves T unchanged and ends the refinement.  The
            refit is ALWAYS accepted.  Open3D leaves refinement to ICP; this step is a least-squares polish on the consensus set, not a
            second search.  At M = 1025 with 30 % true pairs one refit took the pose error from 1.3e-3 to 1.7e-4 while a borderline
            pair may leave the set: a rule "keep only if the count does not fall" would throw the better pose away
transformation: the identity without a winner; fitness = n / K with n the inliers under the final T (Open3D divides by the number of
correspondences), 0 without a winner; inlier_rmse = sqrt(sum / n); status 0 found, 1 no surviving hypothesis with count >= 3, 2 K < 3;
inliers[i] = corr[i] for the final inliers, -1 elsewhere.  Three launches whatever the data, no atomics, no workgroup waits on another,
no allocation inside the library and no host synchronisation: a call can be captured in a hipGraph.  One seed serves every cloud: the
outputs are the same bits run to run, in any batch position and however the hypotheses are split across workgroups.

RANSAC plane segmentation (`segment_plane`, `segment_planes`, `point_plane_distance`).  The dominant plane of a cloud, the floor, the
table or a wall, and the points on it: Open3D's `segment_plane`, PCL's `SACSegmentation` with `SACMODEL_PLANE` (with `axis`:
`SACMODEL_PERPENDICULAR_PLANE`) at a fixed number of hypotheses.  It stands between the filters and `cluster_dbscan`: a support plane
joins every object on it into one cluster.  The route without it is a host loop of `randint` triples, cross products, an (H, N)
distance matrix in chunks, `argmax` and `torch.linalg.eigh`.  Definition (include/gecco_hip.h; tests/_plane_ref.py restates it in
numpy).  Per cloud, with r = fp32(distance_threshold):
    usable  the indices i in ascending order with three finite coordinates and, with `mask`, a non-zero mask entry; K of them
            (`n_points`); c0 = double(the first usable point).  Every later step streams the packed list (x, y, z, bits of i)
    draw    hypothesis h draws three distinct usable points a0, a1, a2 with the generator of `ransac_registration` (above): the same
            bits for the same seed, h and K
    checks  in fp64 on the fp32 coordinates, every operation rounded, none contracted, no division and no root:
            1  degenerate triangle: check 1 of `ransac_registration` on the three points (code 1)
            2  only with `axis` a: n_raw = e1 x e2; rejected (code 2) when (n_raw . a)^2 < (cos2 |n_raw|^2) |a|^2 with
               cos2 = cos(max_angle)^2 formed in double on the host: the angle between normal and axis, either sense, is above max_angle
    plane   of a hypothesis: the fp32 pair (nf, cf), nf = fp32(n_raw / sqrt(|n_raw|^2)) and cf = the point a0 itself: exact, so no
            d = -n . p cancellation happens on a cloud far from the origin
    candidates  given, [a, b, c, d] = candidates[b, h] replaces the draw and check 1; a non-finite entry or a zero normal is code 4;
            check 2 applies to n_raw = abc; s = 1 / sqrt(|abc|^2), nf = fp32(abc s), cf = fp32(-(d s) (abc s)); the triples are -1
    distance  t = ((px - cx) nx + (py - cy) ny) + (pz - cz) nz, every operation rounded to fp32, none contracted; p is an inlier iff
            |t| <= r, so a NaN is never an inlier
    score   count, and the fp64 sum of double(t) double(t) (exact products) over the inliers, accumulated sequentially in list order.
            Per hypothesis, with return_hypotheses: the triple, the (nf, cf) scored (zeros when rejected), count (or -code), sum (or
            +inf).  K < 3: triple -1, count -1, sum +inf
    select  the hypothesis with code 0 and count >= max(3, min_inliers) that is best under (count descending, sum ascending, h
            ascending): the total order of `ransac_registration`, so the way the hypotheses fall into workgroups cannot change it
    refit   refine_passes times on the inliers of the current plane: the fp64 sums about c0 of 1, t^2, d = p - c0 and the six distinct
            entries of d d^T, each thread over its strided points, the wave by a fixed shuffle tree, the waves in order;
            C = S / n - m m^T scaled by its largest magnitude, 8 cyclic Jacobi sweeps over (0, 1), (0, 2), (1, 2) with `icp`'s guarded
            rotation, the eigenvector of the smallest eigenvalue (the lowest index among equals), normalised; the new plane is
            (fp32(n), fp32(c0 + m)).  A pass with fewer than 3 inliers or a result that is not finite leaves the plane unchanged and
            ends the refits.  The refit is ALWAYS accepted, as in `ransac_registration`
    final   the last evaluation gives `inliers`, `n_inliers`, fitness = n_inliers / K and inlier_rmse = sqrt(sum / n_inliers)
    plane   [a, b, c, d] in fp64: the unit normal and d = -n . c with c the fp64 point the last plane passes through.  Sign, the rule
            of `estimate_normals`: with a viewpoint v, n . (v - c) >= 0; without, the component of largest magnitude is positive, the
            lowest axis among equal magnitudes
    status  0 found; 1 no hypothesis reached the inlier bar: plane [0, 0, 1, 0], inliers all false, fitness and rmse 0; 2 K < 3: the
            same outputs, and every hypothesis reports triple -1
Three launches whatever the data: the compaction, the hypothesis kernel (a workgroup per 1024 consecutive hypotheses, which ends by
reducing its own results to ONE 16-byte record, so the workspace is O(B ceil(H / 1024) + B N) and not O(B H)) and select + refit.  No
atomics, no allocation inside the library and no host synchronisation: a call can be captured in a hipGraph.  The outputs are the same
bits run to run, in any batch position and however the hypotheses are split across workgroups.

DBSCAN clustering (`cluster_dbscan`, `cluster_sizes`).  "Which points belong together": the step Open3D (`cluster_dbscan`), PCL
(`EuclideanClusterExtraction`, the same thing with every point a core point) and scikit-learn (`DBSCAN`) put behind the voxel filter
and the outlier filter, before a registration per object.  The route without it is an N x N adjacency matrix (`cdist <= eps`: 10 GB of
booleans at 100 000 points) and a host loop over it.  Definition (include/gecco_hip.h; tests/_dbscan_ref.py restates it in numpy
float32).  Per cloud, with eps2 = fp32(eps * eps) and min_points >= 1:
    dist2      the spelling of `knn`: (dx dx + dy dy) + dz dz, every operation rounded to fp32, none contracted, NaN -> +inf.  It is
               bitwise symmetric; a point with a non-finite coordinate is nobody's neighbour, not even its own
    neighbour  dist2(i, j) <= eps2, inclusive; a finite point is its own neighbour.  count_i = the number of neighbours of i
    core       count_i >= min_points.  The core points form a graph with an edge wherever two of them are neighbours; root_i = the
               lowest index of i's connected component; a component's cluster id is the rank of its root among all roots, ascending
    border     a non-core point with a core neighbour takes the lowest cluster id among its core neighbours
    noise      everything else: -1
The result is unique and equals Open3D's and scikit-learn's label for label (both visit points in index order and finish a cluster
before they open the next).  Points x = 0, 1, 2, 10, 11, 5.5 on a line, eps = 1, min_points = 2: labels [0, 0, 0, 1, 1, -1]; with
min_points = 3 only point 1 is core and the labels are [0, 0, 0, -1, -1, -1].  1 + 2 max_rounds + 2 launches whatever the data: a
count scan, max_rounds rounds of hook (a scan: Shiloach-Vishkin minimum hooking on a forest of stars, integer atomicMin) + compress
(pointer chasing), a border scan and one labelling workgroup per cloud; the scans are `knn`'s loop.  A round that hooks nothing has
found the fixed point (`rounds` counts it, `status` 0) and the cloud's later workgroups return at once; the default limit
ceil(log2 max(N, 2)) + 2 cannot be exceeded; a cloud that runs out of an explicit limit has status 1 and labels that refine the true
clusters.  In every launch what is read is written by no thread of that launch, so labels, rounds and status are the same bits run to
run and in any batch position, also at the limit; no float atomics, no host synchronisation.

Fixed-radius neighbour search (`radius_count`, `radius_search`, `radius_outlier_mask`).  "Every point within r": the query Open3D and
PCL pair with `knn` (`search_radius_vector_3d`, `search_hybrid_vector_3d`, `remove_radius_outlier` / `RadiusOutlierRemoval`) and
PointNet++'s `ball_query`.  The route without it is `metrics.distance_matrix(...) <= r` and `nonzero`: an M x N matrix (40 GB at
100 000 points against themselves) whose aa + bb - 2ab rounding puts pairs at the bound on the wrong side.  Definition
(include/gecco_hip.h; tests/_radius_ref.py restates it in numpy float32).  Per batch element, for queries q_i (i < M) and reference
points p_j (j < N):
    r2         fp32(radius * radius): the fp32 value of the radius squared in double and rounded once, `cluster_dbscan`'s eps2.  The
               radius must be a finite fp32 number > 0 and so must its square
    dist2      the spelling of `knn`: (dx dx + dy dy) + dz dz, every operation rounded to fp32, none contracted, NaN -> +inf
    neighbour  j is a neighbour of i iff dist2(q_i, p_j) <= r2, inclusive, compared on the bits as unsigned integers.  The bound is
               defined on r2 because r and r2 disagree at it: radius = sqrt(2) excludes a pair at dist2 = 2, for
               fp32(fp32(sqrt 2)^2) = 1.99999988.  A non-finite query has no neighbours and a non-finite reference point is nobody's
               neighbour; neither disturbs another row or cloud
    self mode  the query cloud is the reference cloud and exclude_self is set: the pair j == i is skipped by index, not by distance,
               so exact duplicates remain neighbours
    count      count[i] = the number of neighbours of i, never clamped
    order      "index" (the default): a row's neighbours in ascending j.  "distance": by (dist2, j) ascending, the lowest index among
               equal distances, which is `knn`'s order
On the 6 x 6 x 6 integer grid of `knn` above in self mode, radius 1.5: query 0 gets [1, 6, 7, 36, 37, 42] with dist2 [1, 1, 2, 1, 2, 2]
in index order and [1, 6, 36, 7, 37, 42] in distance order (`knn`'s first six; 43 lies at dist2 3 > 2.25), query 215 gets [173, 178,
179, 208, 209, 214], an interior point has 18 neighbours, and without self exclusion every count is one higher.  Radius 1: query 0
gets [1, 6, 36], the bound being inclusive; radius sqrt(2) gives the same three.  Ten identical points, query 3: self mode gives
[0, 1, 2, 4, ..., 9], count 9; without exclusion all ten.
One scan kernel (`knn`'s direct loop: one thread per query, the reference cloud streamed through LDS) in three modes: the counts; the
CSR fill, which is handed the exclusive prefix sum of the counts and recounts each row by the same predicate, so it writes exactly
count[r] entries; the fixed-width fill, which writes the first K neighbours, pads with -1 / +inf and reports the unclamped count from
the same pass.  A thread writes its own words only: no atomics, no workspace, the same bits run to run and in any batch position.
There is no split form: few queries against many points (2048 against 100 000: 32 workgroups) leave most of the device idle.

The grid index of the radius operators (`build_grid_index`, `GridIndex`, the `index=` keyword; csrc/grid.hip, gecco_grid_keys_f32,
gecco_grid_build_f32, gecco_grid_radius_count_f32, gecco_grid_radius_search_f32).  The scan above tests all N reference points for
every query; at 100 000 points and 38.6 neighbours per point that is 100 000 candidates where the cells within reach hold about 250.
Definition (include/gecco_hip.h; tests/_grid_ref.py restates it in numpy float32):
    cell       `voxel_downsample`'s for voxel_size = cell_size, same roundings and the same 63-bit key.  A point that filter would drop
               (a non-finite u, a cell outside [-2^20, 2^20)) is OFF-GRID: its key is bit 63 alone, which no real key has
    sorted     a stable torch.sort of the keys as unsigned integers: cells in ascending key, a cell's points in ascending original
               index, the off-grid points last (the tail).  perm[s] = the original index at position s; sorted_points[s] = (x, y, z,
               the bits of perm[s]); an open-addressing table (the hash and the load <= 0.5 of `voxel_downsample`) maps a key to its
               run [start, end) of positions; n_in_grid = where the tail starts
    query      with R the least fp32 number >= sqrt(r2 (1 + 2^-23) + 2^-149) (1 + 2^-16), per axis the cells cell(fp32(q - R)) ..
               cell(fp32(q + R)), clamped to the grid, x outermost and z innermost (ascending key), then the tail.  radius <=
               cell_size makes that box at most 4 cells wide per axis wherever fp32 resolves the coordinates inside a cell; a wider
               box is answered by a scan of all N sorted positions.  The cells are a filter only: j is a neighbour iff dist2(q, p_j)
               <= r2 on the bits, the predicate above, so counts, neighbours and dist2 are the direct form's bit for bit
               (csrc/grid.hip proves that no neighbour lies outside the box)
    order      "index" and "distance" as above, after one torch.sort more; "grid": the row as filled, ascending position in the
               sorted order = by (cell key, j), tail last
On the 6 x 6 x 6 grid above with cell_size = 1.5 (coordinates {0, 1 | 2 | 3, 4 | 5} share a cell per axis), radius 1.5, self mode:
query 0's six neighbours lie in its own cell and its grid-order row is [1, 6, 7, 36, 37, 42]; query 43 = (1, 1, 1) gets [1, 6, 7, 36,
37, 42, 8, 38, 44, 13, 48, 49, 50, 73, 78, 79, 80, 85]: cell (0, 0, 0) first, then (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), ...
One thread per query, answered in the order of the index so that a wave reads the same cells; a thread writes its own words only, no
atomics, no workspace, the same bits run to run and in any batch position.  Nothing takes the grid by default: the caller asks for it.

ISS keypoints (`iss_keypoints`, `ISSResult`, `cloud_resolution`; csrc/iss.hip, gecco_iss_keypoints_f32).  The detector Open3D
(`compute_iss_keypoints`) and PCL (`ISSKeypoint3D`) put in front of the descriptor (Intrinsic Shape Signatures, Zhong 2009): keep
the points whose neighbourhood is not flat, not a line and not isotropic, and thin them by non-maximum suppression, so that `fpfh`,
`match_features` and `ransac_registration` work on hundreds of points instead of all N.  The route without it is `radius_search` into
a CSR list, `repeat_interleave` and `index_add` (float atomics) for the moments, `torch.linalg.eigvalsh` on N little matrices, and a
second `radius_search` with a `scatter_reduce`: two host synchronisations and two materialised neighbour lists.  Here a thread walks
the cells of the grid index its ball can reach (csrc/grid_walk.h: the walk `radius_count(index=...)` makes, one spelling for both) and
pools in registers.  Definition (include/gecco_hip.h; tests/_iss_ref.py restates
it in numpy).  Per cloud, with r2s = fp32(salient_radius^2) and r2n = fp32(non_max_radius^2) formed as `radius_count` forms r2:
    ball       B_r(i) = the j with dist2(p_i, p_j) <= r2 on the bits, `radius_count`'s predicate, the point itself INCLUDED by index
               (Open3D's radius search returns the query).  A non-finite point is in nobody's ball, not even its own.  The ball is
               visited in ascending sorted position of the index (by (cell key, j), the off-grid tail last): that order is part of
               the definition, as it is of order="grid"
    count      m_i = |B_r2s(i)|
    moments    in fp64 on the fp32 coordinates, about the point itself, every operation rounded and none contracted:
               d = double(p_j) - double(p_i) per axis;  S1 = sum d (3 sums), S2 = sum d d^T (xx, xy, xz, yy, yz, zz), each from 0 in
               ball order;  inv = 1 / m;  mu = S1 inv;  C_ab = S2_ab inv - mu_a mu_b.  |d| <= the radius, so the raw moments cancel
               against the radius and not against the cloud's distance from the origin
    eigen      big = max |C_ab|;  A = C sc with sc = 1 / big;  8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with the guarded
               rotation of `icp` (a fixed count), none of its operations contracted;  lambda = diag big, negative roundings clamped
               to 0, sorted lambda0 <= lambda1 <= lambda2
    candidate  m_i >= min_neighbors, big a positive finite number (all of the ball identical: not a candidate, Open3D's
               cov.isZero()), lambda1 < gamma_21 lambda2, lambda0 < gamma_32 lambda1 (fp64 products, no division) and lambda0 > 0.
               saliency_i = lambda0 for a candidate, 0 otherwise;  eigenvalues_i = 0 where m_i < min_neighbors or big is not a
               positive finite number
    keypoint   i is a candidate, |B_r2n(i)| >= min_neighbors, and no j in B_r2n(i) has saliency_j > saliency_i (fp64 compare).  Equal
               saliencies keep each other, as Open3D's IsLocalMaxima does: two exact duplicates of a keypoint are both kept
`counts` is m_i; `n_keypoints` the row sum of the mask.  A point's result depends on the cloud and on the index's cell_size and
origin, which fix the order of the sums, and on nothing else: the same bits run to run, in any batch position and at any workgroup
size; an index built for the call and a prebuilt one with the same parameters give the same bits; two indices with different cells
may differ in the last bits of the eigenvalues.
On the 6 x 6 x 6 integer grid above with both radii 1.5 (cell_size 1.5) and the defaults: point 0, a corner, has m = 7, C = 12/49 on
the diagonal and -2/49 off it and lambda = (8/49, 2/7, 2/7): lambda1 = lambda2, not a candidate.  Point 1 = (0, 0, 1), on an edge: m =
10, lambda = (0.18, 0.3, 0.6), saliency 0.18.  Point 7 = (0, 1, 1), on a face: m = 14, lambda1 = lambda2 = 4/7.  Point 43 = (1, 1, 1):
m = 19, lambda = 10/19 three times.  The candidates are the 48 points inside the 12 edges, saliency 0.18 each up to rounding in the
last place; all 48 are keypoints and nothing else is.
Two launches, one thread per sorted position: the saliency of every point, then the selection; a thread writes its own words only, no
atomics, no workspace.  `cloud_resolution` is Open3D's ComputeModelResolution, the mean distance to the nearest other point.
HIP tensors only: there is no CPU fallback (`voxel_pool`, `cluster_sizes` and `point_plane_distance`, plain torch, run on any device)."""
from __future__ import annotations

import ctypes as C
import math
import operator
from typing import NamedTuple

import torch
from torch import Tensor

from . import _lib
from .hip_ops import _ptr, _stream

FPS_RESIDENT_MAX_POINTS = 8192   # GECCO_FPS_RESIDENT_MAX_POINTS: 1024 threads * 8 points in registers
_FPS_STREAM_SLICE = 1024         # GECCO_FPS_STREAM_SLICE: points per workgroup of the streaming form
_FPS_FORMS = {None: 0, "resident": 1, "streaming": 2}
KNN_MAX_K = 64                   # GECCO_KNN_MAX_K
KNN_SPLIT_SLICE = 4096           # GECCO_KNN_SPLIT_SLICE: reference points per slice of the split form
_KNN_FORMS = {None: 0, "direct": 1, "split": 2}
VOXEL_MAX_POINTS = 1 << 30       # GECCO_VOXEL_MAX_POINTS
ICP_MAX_ITERATIONS = 1000        # GECCO_ICP_MAX_ITERATIONS
_ICP_STATE_BYTES = 160           # GECCO_ICP_STATE_BYTES
_ICP_METHODS = {"point_to_point": 0, "point_to_plane": 1}
FPFH_BINS = 33                   # GECCO_FPFH_BINS
FEATURE_MAX_DIM = 64             # GECCO_FEATURE_MAX_DIM
RANSAC_MAX_HYPOTHESES = 1 << 24  # GECCO_RANSAC_MAX_HYPOTHESES
RANSAC_MAX_REFINE = 8            # GECCO_RANSAC_MAX_REFINE
_RANSAC_BLOCK_HYPOTHESES = 1024  # GECCO_RANSAC_BLOCK_HYPOTHESES
DBSCAN_MAX_ROUNDS = 64            # GECCO_DBSCAN_MAX_ROUNDS
PLANE_MAX_HYPOTHESES = 1 << 24   # GECCO_PLANE_RANSAC_MAX_HYPOTHESES
PLANE_MAX_REFINE = 8             # GECCO_PLANE_RANSAC_MAX_REFINE
_PLANE_BLOCK_HYPOTHESES = 1024   # GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES


def _fps_workspace_bytes(B: int, N: int) -> int:
    """GECCO_FPS_WORKSPACE_BYTES(B, N)"""
    return ((4 * B * N + 7) & ~7) + 16 * B * ((N + _FPS_STREAM_SLICE - 1) // _FPS_STREAM_SLICE)


def _cloud(points: Tensor):
    single = points.dim() == 2
    p = points[None] if single else points
    if p.dim() != 3 or p.shape[2] != 3 or not p.is_floating_point():
        raise ValueError("expected a floating cloud of shape (B, N, 3) or (N, 3)")
    return p, single


def _vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _f32(t: Tensor):
    """the fp32 contiguous copy the library reads, detached, and its device pointer"""
    x = t.detach().float().contiguous()
    return x, _ptr(x)   # HIP tensors only: there is no CPU fallback


def _same_batching(a: Tensor, a_single: bool, b: Tensor, b_single: bool, a_name: str, b_name: str):
    if b_single != a_single:
        raise ValueError(f"{a_name} and {b_name} must both be batched (B, ., 3) or both single (., 3)")
    if b.shape[0] != a.shape[0]:
        raise ValueError(f"{a_name} has {a.shape[0]} clouds, {b_name} has {b.shape[0]}")


def _check_form(form):
    if form not in _KNN_FORMS:
        raise ValueError("form must be None, 'direct' or 'split'")


def _positive_f32(value, name: str, catch):
    """`value` rounded to fp32, as it reaches the library; `catch`: what float() may raise for something that is not a number"""
    try:
        v = C.c_float(float(value)).value
    except catch as e:
        raise ValueError(f"{name} = {value!r} is not a number") from e
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} = {value!r} must be a finite fp32 number > 0")
    return v


def _integer(value, name: str) -> int:
    """`value` as a Python int; ValueError for anything that is not an integer (a float, also a whole one, a string, a bool)"""
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError as e:
        raise ValueError(f"{name} = {value!r} is not an integer") from e


def _refits_and_seed(refine_passes, seed, max_refine: int, slots: int = 1):
    """refine_passes in 0 .. max_refine and a seed that `slots` consecutive calls can count up from, as Python ints"""
    refine_passes = _integer(refine_passes, "refine_passes")
    if not 0 <= refine_passes <= max_refine:
        raise ValueError(f"refine_passes = {refine_passes} is not in 0 .. {max_refine}")
    seed = _integer(seed, "seed")
    if not 0 <= seed <= (1 << 64) - slots:
        raise ValueError(f"seed = {seed} is not in 0 .. 2^64 - {slots}")
    return refine_passes, seed


def _candidates_or_count(candidates, hypotheses, trailing: tuple, default: int, limit: int, B: int, single: bool):
    """`candidates` (numbers or a tensor, (H, *trailing) or (B, H, *trailing)) or `hypotheses`, never both: the candidates as a tensor
    (or None) and H in 1 .. limit (`default` when neither is given)"""
    if candidates is None:
        H = default if hypotheses is None else _integer(hypotheses, "hypotheses")
    else:
        if hypotheses is not None:
            raise ValueError("candidates set the number of hypotheses: pass one of `hypotheses` and `candidates`")
        shape, d = ", ".join(str(n) for n in trailing), len(trailing)
        try:
            candidates = candidates if isinstance(candidates, Tensor) else torch.as_tensor(candidates, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"candidates must be (H, {shape}) or ({B}, H, {shape})") from e
        if candidates.is_complex() or candidates.dtype == torch.bool or candidates.dim() not in (d + 1, d + 2) or \
                tuple(candidates.shape[-d:]) != trailing or (candidates.dim() == d + 2 and (single or candidates.shape[0] != B)):
            raise ValueError(f"candidates must be (H, {shape}){'' if single else f' or ({B}, H, {shape})'}")
        H = int(candidates.shape[-d - 1])
    if not 1 <= H <= limit:
        raise ValueError(f"hypotheses = {H} is not in 1 .. {limit}")
    return candidates, H


def _per_cloud_vector(value, name: str, B: int, refuse_bool: bool):
    """numbers or a tensor of shape (3,) or (B, 3), as a tensor (the caller moves it to the device and expands it)"""
    v = torch.as_tensor(value)
    if v.is_complex() or (refuse_bool and v.dtype == torch.bool) or tuple(v.shape) not in ((3,), (B, 3)):
        raise ValueError(f"{name} must be (3,) or ({B}, 3)")
    return v


def _unbatch(out, single: bool):
    """drop the batch dimension of every tensor of `out` for single clouds (None stays None)"""
    return [None if t is None else t[0] for t in out] if single else out


def _fps(p: Tensor, k: int, start, want_sel2: bool, form):
    """p (B, N, 3) of any float dtype / strides -> idx (B, k) int32, sel2 (B, k) fp32 or None"""
    B, N, _ = p.shape
    k = int(k)
    if form not in _FPS_FORMS:
        raise ValueError("form must be None, 'resident' or 'streaming'")
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    if B < 1:
        raise ValueError("empty batch")
    if k > N:
        raise ValueError(f"k = {k} above the {N} points of a cloud")
    fits = N <= FPS_RESIDENT_MAX_POINTS
    if form == "resident" and not fits:
        raise ValueError(f"the resident form takes N <= {FPS_RESIDENT_MAX_POINTS} points (got {N})")
    code = 1 if (form == "resident" or (form is None and fits)) else 2
    if isinstance(start, Tensor) and (start.dim() != 1 or start.shape[0] != B or start.is_floating_point() or start.is_complex()):
        raise ValueError(f"start must be an int or an integer tensor of shape ({B},)")
    x, px = _f32(p)
    if isinstance(start, Tensor):
        st = start.to(device=x.device, dtype=torch.int32).contiguous()
    else:
        st = None if int(start) == 0 else torch.full((B,), int(start), device=x.device, dtype=torch.int32)
    idx = torch.empty(B, k, device=x.device, dtype=torch.int32)
    sel2 = torch.empty(B, k, device=x.device, dtype=torch.float32) if want_sel2 else None
    ws = torch.empty(_fps_workspace_bytes(B, N), device=x.device, dtype=torch.uint8) if code == 2 else None
    _lib.check(_lib.load().gecco_fps_f32(px, _vp(st), _vp(idx), _ptr(sel2), _vp(ws), B, N, k, code, _stream()), "gecco_fps_f32")
    return idx, sel2


def farthest_point_sample(points: Tensor, k: int, start=0, return_distances: bool = False, form: str | None = None):
    """Indices of k farthest-point samples of each cloud (module docstring: the definition).  points (B, N, 3) or (N, 3) on the HIP device,
    any float dtype and strides (computed on an fp32 contiguous copy); start: an int, or a (B,) integer tensor of per-cloud start indices
    (clamped into [0, N) on the device).  Returns idx, int64 (B, k) — (k,) for a single cloud — with idx[:, 0] = start; with
    return_distances also dist, fp32 of the same shape: the distance of each pick to the picks before it (+inf in column 0, non-increasing
    after).  form None: resident while N <= FPS_RESIDENT_MAX_POINTS, streaming above; "resident" (ValueError above the limit) or "streaming"
    force one — same indices either way.  ValueError for k < 1 or k > N; GeccoHipError for CPU tensors.  No gradient: indices."""
    p, single = _cloud(points)
    idx, sel2 = _fps(p, k, start, return_distances, form)
    out = [idx.long()]
    if return_distances:
        out.append(sel2.sqrt())
    out = _unbatch(out, single)
    return tuple(out) if return_distances else out[0]


def farthest_point_subsample(points: Tensor, k: int, start=0, form: str | None = None) -> Tensor:
    """The k farthest-point samples themselves: points gathered along `farthest_point_sample`'s indices, (B, k, 3) — (k, 3) for a single
    cloud — in the input's dtype.  The gather is a plain torch gather, so gradients flow to the kept points (and only to them)."""
    p, single = _cloud(points)
    idx, _ = _fps(p, k, start, False, form)
    out = p.gather(1, idx.long()[:, :, None].expand(-1, -1, 3))
    return out[0] if single else out


def _knn_workspace_bytes(B: int, M: int, N: int, k: int) -> int:
    """GECCO_KNN_WORKSPACE_BYTES(B, M, N, k)"""
    return 8 * B * M * k * ((N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE)


def _knn(q: Tensor, r: Tensor | None, k: int, exclude_self: bool, want_d2: bool, form):
    """q (B, M, 3), r (B, N, 3) or None (= q) of any float dtype / strides -> idx (B, M, k) int32, d2 (B, M, k) fp32 or None"""
    _check_form(form)
    B, M, _ = q.shape
    k = int(k)
    if r is not None and r.shape[0] != B:
        raise ValueError(f"query has {B} clouds, ref has {r.shape[0]}")
    N = M if r is None else r.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if exclude_self and M != N:
        raise ValueError(f"exclude_self needs the query cloud to be the reference cloud (M = {M}, N = {N})")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k} is not in 1 .. {KNN_MAX_K}")
    if k > N - int(exclude_self):
        raise ValueError(f"k = {k} above the {N - int(exclude_self)} candidates of a query")
    x, px = _f32(q)
    y, py = (x, px) if r is None or r is q else _f32(r)
    idx = torch.empty(B, M, k, device=x.device, dtype=torch.int32)
    d2 = torch.empty(B, M, k, device=x.device, dtype=torch.float32) if want_d2 else None
    # a workspace is offered where knn_launch's auto rule can take the split form; the library decides
    slices = (N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE
    offer = form == "split" or (form is None and slices > 1
                                and B * ((M + 63) // 64) < torch.cuda.get_device_properties(x.device).multi_processor_count)
    ws = torch.empty(_knn_workspace_bytes(B, M, N, k), device=x.device, dtype=torch.uint8) if offer else None
    _lib.check(_lib.load().gecco_knn_f32(px, py, _vp(idx), _ptr(d2), _vp(ws), B, M, N, k, int(bool(exclude_self)), _KNN_FORMS[form],
                                         _stream()), "gecco_knn_f32")
    return idx, d2


def knn(query: Tensor, ref: Tensor | None = None, k: int = 16, exclude_self: bool | None = None, return_distances: bool = True,
        form: str | None = None):
    """The k nearest points of `ref` to every point of `query` (module docstring: the definition).  query (B, M, 3) or (M, 3), ref
    (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies).  ref=None: the query cloud
    itself, and exclude_self then defaults to True (a point is not its own neighbour); with a ref it defaults to False.  Returns idx, int64
    (B, M, k) — (M, k) for single clouds — and, with return_distances, dist = sqrt(dist2), fp32 of the same shape, non-decreasing along
    k.  form None / "direct" / "split": same bits either way.  ValueError for bad shapes, k outside 1 .. KNN_MAX_K or above the candidates
    of a query, mismatched batch sizes, exclude_self with a ref of another size, an unknown form; GeccoHipError for CPU tensors.  No
    gradient: indices (and the distances are detached)."""
    q, single = _cloud(query)
    r = None
    if ref is not None:
        r, rsingle = _cloud(ref)
        if rsingle != single:   # (_knn compares the cloud counts, after the form: not _same_batching)
            raise ValueError("query and ref must both be batched (B, ., 3) or both single (., 3)")
    if exclude_self is None:
        exclude_self = ref is None
    idx, d2 = _knn(q, r, k, bool(exclude_self), return_distances, form)
    out = [idx.long()]
    if return_distances:
        out.append(d2.sqrt())
    out = _unbatch(out, single)
    return tuple(out) if return_distances else out[0]


def knn_gather(values: Tensor, idx: Tensor) -> Tensor:
    """values (B, N, C) gathered along idx (B, M, k) of `knn` -> (B, M, k, C): out[b, i, t] = values[b, idx[b, i, t]].  A plain torch
    gather, so gradients flow to the gathered rows (a row's gradient is summed over every (i, t) that picked it)."""
    if values.dim() != 3 or idx.dim() != 3 or idx.shape[0] != values.shape[0] or idx.is_floating_point() or idx.is_complex():
        raise ValueError("expected values (B, N, C) and integer idx (B, M, k)")
    if not values.is_cuda or not idx.is_cuda:
        raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")
    B, M, k = idx.shape
    Cn = values.shape[2]
    return values.gather(1, idx.long().reshape(B, M * k, 1).expand(-1, -1, Cn)).view(B, M, k, Cn)


def statistical_outlier_mask(points: Tensor, k: int = 16, std_ratio: float = 2.0, return_scores: bool = False):
    """The statistical outlier filter of PCL / Open3D on `knn`: score_i = the mean distance of point i to its k nearest neighbours (itself
    excluded); per cloud keep_i = score_i <= mean(score) + std_ratio * std(score), the sample standard deviation.  points (B, N, 3) or
    (N, 3) -> a bool mask (B, N) or (N,), True for the points to keep; with return_scores also the fp32 scores of the same shape."""
    p, single = _cloud(points)
    _, d2 = _knn(p, None, k, True, True, None)
    score = d2.sqrt().mean(-1)
    keep = score <= score.mean(-1, keepdim=True) + float(std_ratio) * score.std(-1, keepdim=True)
    keep, score = _unbatch([keep, score], single)
    return (keep, score) if return_scores else keep


def estimate_normals(points: Tensor, k: int = 16, radius: float | None = None, viewpoint=None, query: Tensor | None = None,
                     idx: Tensor | None = None, return_curvature: bool = False, return_eigenvalues: bool = False,
                     return_count: bool = False, form: str | None = None):
    """Unit normals of the surface that `points` samples, from the PCA of k-neighbourhoods (module docstring: the definition).  points
    (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on an fp32 contiguous copy).  query None: the normals at
    the points themselves; or (B, M, 3) / (M, 3): at other positions (the 2048 farthest-point samples of a 100 000-point cloud).  The
    search is `knn` of the queries in `points` with the point itself among the candidates, through `form` (None / "direct" / "split":
    same bits).  idx: the int64 or int32 (B, M, k) — (M, k) for single clouds — indices a caller already holds from
    `knn(query, points, k, exclude_self=False)`; the search is skipped, k is idx's last dimension and the distances a radius needs are
    recomputed from the coordinates, with the search's own roundings.  radius: only neighbours within it count (hybrid search); viewpoint
    (3,) or (B, 3), numbers or a tensor: normals point towards it.  Returns normals, fp32 (B, M, 3) or (M, 3), then the extras asked
    for, in the order curvature fp32 (B, M), eigenvalues fp32 (B, M, 3) ascending, count int64 (B, M).  ValueError for bad shapes, k
    outside 1 .. KNN_MAX_K or above N, a radius that is not > 0, an idx whose shape disagrees with the clouds, mixed batched and single
    inputs, an unknown form; GeccoHipError for CPU tensors.  No gradient: the inputs are detached."""
    p, single = _cloud(points)
    q = None
    if query is not None:
        q, qsingle = _cloud(query)
        _same_batching(p, single, q, qsingle, "points", "query")
    _check_form(form)
    B, N, _ = p.shape
    M = N if q is None else q.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if idx is not None:
        if not isinstance(idx, Tensor) or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
            raise ValueError("idx must be an integer tensor")
        if idx.dim() != (2 if single else 3):
            raise ValueError("idx must be (M, k) for single clouds and (B, M, k) for batched ones")
        ix = idx[None] if single else idx
        if ix.shape[0] != B or ix.shape[1] != M:
            raise ValueError(f"idx of shape {tuple(idx.shape)} does not belong to {B} clouds of {M} queries")
        k = ix.shape[2]
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k} is not in 1 .. {KNN_MAX_K}")
    if k > N:
        raise ValueError(f"k = {k} above the {N} points of a cloud")
    radius2 = 0.0   # no radius
    if radius is not None:
        radius = float(radius)
        if not radius > 0:
            raise ValueError(f"radius = {radius} must be > 0")
        radius2 = radius * radius   # rounded to fp32 on its way into the library
    vw = None if viewpoint is None else _per_cloud_vector(viewpoint, "viewpoint", B, refuse_bool=False)
    x, px = _f32(p)
    y, py = (x, px) if q is None else _f32(q)
    if idx is None:
        ix, d2 = _knn(y, x, k, False, radius is not None, form)
    else:
        if not ix.is_cuda:
            raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")
        ix, d2 = ix.detach().to(device=x.device, dtype=torch.int32).contiguous(), None
    if vw is not None:
        vw = vw.detach().to(device=x.device, dtype=torch.float32).expand(B, 3).contiguous()
    normals = torch.empty(B, M, 3, device=x.device, dtype=torch.float32)
    curv = torch.empty(B, M, device=x.device, dtype=torch.float32) if return_curvature else None
    eig = torch.empty(B, M, 3, device=x.device, dtype=torch.float32) if return_eigenvalues else None
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32) if return_count else None
    _lib.check(_lib.load().gecco_normals_f32(px, py, _vp(ix), _ptr(d2), _ptr(vw), radius2, _vp(normals), _ptr(eig), _ptr(curv), _vp(cnt),
                                             B, M, N, k, _stream()), "gecco_normals_f32")
    out = [normals]
    if return_curvature:
        out.append(curv)
    if return_eigenvalues:
        out.append(eig)
    if return_count:
        out.append(cnt.long())
    out = _unbatch(out, single)
    return out[0] if len(out) == 1 else tuple(out)


def _voxel_workspace_bytes(B: int, N: int) -> int:
    """GECCO_VOXEL_WORKSPACE_BYTES(B, N): 16 bytes per table slot (the power of two >= 2 N of them per cloud), 36 per point, 4 per cloud"""
    cap = 1 << (2 * N - 1).bit_length()
    return (B * (16 * cap + 36 * N + 4) + 7) & ~7


def voxel_downsample(points: Tensor, voxel_size: float, origin=None, max_voxels: int | None = None, return_index: bool = False,
                     return_counts: bool = False, return_inverse: bool = False):
    """The voxel-grid filter: one point per occupied cell of a grid of edge `voxel_size`, at the centroid of the cell's points (module
    docstring: the definition).  points (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on an fp32
    contiguous copy); origin (3,) or (B, 3), numbers or a tensor: the grid's anchor (default 0).  Returns centroids, fp32 (B, V, 3), and
    n_voxels, int64 (B,), then the extras asked for, in the order first int64 (B, V) (the lowest point index of each voxel), count int64
    (B, V), inverse int64 (B, N) (the voxel of each point, -1 for a dropped one); for a single cloud the batch dimension is dropped
    (n_voxels is then a 0-d tensor).  Voxels are numbered by first occurrence.  max_voxels None: the function reads n_voxels.max() once —
    its only host synchronisation — and trims the outputs to V = max(that, 1) rows; rows at or after a cloud's n_voxels are zero with
    count = 0 and first = -1.  max_voxels given (1 .. N): no synchronisation, V = max_voxels, the call can be captured in a hipGraph;
    points of voxels numbered max_voxels or higher get inverse = -1 and n_voxels is reported unclamped.  ValueError for bad shapes, a
    voxel_size that is not a finite fp32 number > 0, max_voxels outside 1 .. N, an origin of the wrong shape; GeccoHipError for CPU
    tensors.  No gradient: the outputs are detached (`voxel_pool(points, inverse, V)` is the differentiable centroid)."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    size = _positive_f32(voxel_size, "voxel_size", (TypeError, OverflowError))
    if max_voxels is not None:
        max_voxels = int(max_voxels)
        if not 1 <= max_voxels <= N:
            raise ValueError(f"max_voxels = {max_voxels} is not in 1 .. {N}")
    org = None if origin is None else _per_cloud_vector(origin, "origin", B, refuse_bool=True)
    x, px = _f32(p)
    if org is not None:
        org = org.detach().to(device=x.device, dtype=torch.float32).expand(B, 3).contiguous()
    V = N if max_voxels is None else max_voxels
    cen = torch.empty(B, V, 3, device=x.device, dtype=torch.float32)
    nv = torch.empty(B, device=x.device, dtype=torch.int32)
    first = torch.empty(B, V, device=x.device, dtype=torch.int32) if return_index else None
    cnt = torch.empty(B, V, device=x.device, dtype=torch.int32) if return_counts else None
    inv = torch.empty(B, N, device=x.device, dtype=torch.int32) if return_inverse else None
    ws = torch.empty(_voxel_workspace_bytes(B, N), device=x.device, dtype=torch.uint8)   # filled by the library, inside the call
    _lib.check(_lib.load().gecco_voxel_downsample_f32(px, _ptr(org), size, _vp(cen), _vp(first), _vp(cnt), _vp(inv), _vp(nv), _vp(ws), B, N, V,
                                                      _stream()), "gecco_voxel_downsample_f32")
    if max_voxels is None:
        V = max(int(nv.max()), 1)   # the one synchronisation
        cen = cen[:, :V].contiguous()
        first = None if first is None else first[:, :V]
        cnt = None if cnt is None else cnt[:, :V]
    out = [cen, nv.long()]
    if return_index:
        out.append(first.long())
    if return_counts:
        out.append(cnt.long())
    if return_inverse:
        out.append(inv.long())
    return tuple(_unbatch(out, single))


def voxel_pool(values: Tensor, inverse: Tensor, n_voxels, reduce: str = "mean") -> Tensor:
    """Per-point attributes pooled onto the voxels of `voxel_downsample`: values (B, N, C) or (N, C), inverse (B, N) or (N,) as
    `return_inverse` gives it -> (B, V, C) or (V, C) in the dtype of `values`, the mean (or, reduce="sum", the sum) of the rows of each
    voxel.  n_voxels: V as an int (the row count of the downsampled cloud; use it inside a graph), or the n_voxels tensor, which is read
    on the host (V = max(n_voxels.max(), 1), as `voxel_downsample` trims).  Rows with inverse = -1 (dropped points, overflow voxels) or
    >= V are skipped; a voxel without points is 0.  Plain torch (`index_add`) on any device, so gradients flow to `values`: this is the
    differentiable route — `voxel_pool(points, inverse, V)` is the differentiable centroid, and normals, colours or features are pooled
    the same way.  It is a float scatter: unlike the kernel's centroids it is NOT bit-reproducible on the device (float atomics), and
    it carries the rounding of an fp32 running sum."""
    if reduce not in ("mean", "sum"):
        raise ValueError("reduce must be 'mean' or 'sum'")
    if not isinstance(values, Tensor) or not isinstance(inverse, Tensor) or not values.is_floating_point():
        raise ValueError("expected floating values (B, N, C) or (N, C) and an integer inverse (B, N) or (N,)")
    if inverse.is_floating_point() or inverse.is_complex() or inverse.dtype == torch.bool:
        raise ValueError("inverse must be an integer tensor")
    single = values.dim() == 2
    val = values[None] if single else values
    inv = inverse[None] if single else inverse
    if val.dim() != 3 or inv.dim() != 2 or inv.shape != val.shape[:2]:
        raise ValueError(f"values of shape {tuple(values.shape)} and inverse of shape {tuple(inverse.shape)} do not belong together")
    V = max(int(n_voxels.max()), 1) if isinstance(n_voxels, Tensor) else int(n_voxels)
    if V < 1:
        raise ValueError(f"V = {V} must be >= 1")
    B, N, Cn = val.shape
    inv = inv.to(device=val.device, dtype=torch.long)
    rows = torch.where((inv >= 0) & (inv < V), inv, V) + (V + 1) * torch.arange(B, device=val.device)[:, None]   # row V of a cloud: skipped
    out = torch.zeros(B * (V + 1), Cn, device=val.device, dtype=val.dtype).index_add(0, rows.reshape(-1), val.reshape(B * N, Cn))
    if reduce == "mean":
        n = torch.zeros(B * (V + 1), device=val.device, dtype=val.dtype).index_add(
            0, rows.reshape(-1), torch.ones(B * N, device=val.device, dtype=val.dtype))
        out = out / n.clamp(min=1)[:, None]
    out = out.view(B, V + 1, Cn)[:, :V]
    return out[0] if single else out


class ICPResult(NamedTuple):
    """What `icp` returns (module docstring: the definition).  status 0: converged, 1: max_iterations reached, 2: too few inliers or a
    singular system, 3: a non-finite `init`."""
    transformation: Tensor          # float64 (B, 4, 4): maps source onto target
    fitness: Tensor                 # fp32 (B,): inliers / M at the last pass
    inlier_rmse: Tensor             # fp32 (B,)
    iterations: Tensor              # int64 (B,): the pass that stopped
    status: Tensor                  # int64 (B,)
    correspondence: Tensor | None   # int64 (B, M): the target index of each source point, -1 without one within the distance


def _icp_workspace_bytes(B: int, M: int, N: int) -> int:
    """GECCO_ICP_WORKSPACE_BYTES(B, M, N)"""
    return _ICP_STATE_BYTES * B + 8 * B * M * ((N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE)


def icp(source: Tensor, target: Tensor, max_correspondence_distance: float, init=None, method: str = "point_to_point",
        target_normals: Tensor | None = None, max_iterations: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
        return_correspondence: bool = False, form: str | None = None) -> ICPResult:
    """Rigid ICP registration of `source` onto `target` (module docstring: the definition).  source (B, M, 3) or (M, 3), target (B, N, 3)
    or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies).  method "point_to_point" or
    "point_to_plane"; the latter needs target_normals, (B, N, 3) or (N, 3) (what `estimate_normals(target)` returns), which the former
    refuses.  init: (4, 4) or (B, 4, 4), numbers or a tensor, the starting transformation (default: the identity).  max_iterations in
    0 .. ICP_MAX_ITERATIONS; 0 only evaluates `init` (Open3D's evaluate_registration).  form None / "direct" / "split": the forms of `knn`,
    same bits either way.  Returns an ICPResult: transformation float64 (B, 4, 4), fitness and inlier_rmse fp32 (B,), iterations and
    status int64 (B,), correspondence int64 (B, M) with return_correspondence and None without; for single clouds the batch dimension is
    dropped.  The call makes 2 * (max_iterations + 1) launches and never synchronises: it can be captured in a hipGraph.  ValueError,
    before any device call, for bad shapes, mixed batched and single inputs, mismatched batch sizes, an unknown method or form, normals
    that are missing, unexpected or mis-shaped, a distance that is not a finite fp32 number > 0, max_iterations out of range, a
    tolerance that is negative or NaN, an init of the wrong shape; GeccoHipError for CPU tensors.  No gradient: the inputs are detached
    (`transform_points` is the differentiable way to apply the result)."""
    s, single = _cloud(source)
    t, tsingle = _cloud(target)
    _same_batching(s, single, t, tsingle, "source", "target")
    B, M, _ = s.shape
    N = t.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if method not in _ICP_METHODS:
        raise ValueError("method must be 'point_to_point' or 'point_to_plane'")
    _check_form(form)
    nrm = None
    if method == "point_to_plane":
        if target_normals is None:
            raise ValueError("method 'point_to_plane' needs target_normals")
        if not isinstance(target_normals, Tensor):
            raise ValueError("target_normals must be a tensor")
        nrm, nsingle = _cloud(target_normals)
        if nsingle != single or nrm.shape != t.shape:
            raise ValueError(f"target_normals of shape {tuple(target_normals.shape)} do not belong to a target of shape {tuple(target.shape)}")
    elif target_normals is not None:
        raise ValueError("target_normals are only used by method 'point_to_plane'")
    r = _positive_f32(max_correspondence_distance, "max_correspondence_distance", (TypeError, ValueError, OverflowError))
    max_iterations = int(max_iterations)
    if not 0 <= max_iterations <= ICP_MAX_ITERATIONS:
        raise ValueError(f"max_iterations = {max_iterations} is not in 0 .. {ICP_MAX_ITERATIONS}")
    relative_fitness, relative_rmse = float(relative_fitness), float(relative_rmse)
    if not relative_fitness >= 0 or not relative_rmse >= 0:
        raise ValueError("relative_fitness and relative_rmse must be >= 0")
    T0 = None
    if init is not None:
        try:
            T0 = init if isinstance(init, Tensor) else torch.as_tensor(init, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"init must be (4, 4) or ({B}, 4, 4)") from e
        if T0.is_complex() or T0.dtype == torch.bool or tuple(T0.shape) not in ((4, 4), (B, 4, 4)):
            raise ValueError(f"init must be (4, 4) or ({B}, 4, 4)")
    x, px = _f32(s)
    y, py = _f32(t)
    nrm, pn = (None, None) if nrm is None else _f32(nrm)
    if T0 is not None:
        T0 = T0.detach().to(device=x.device, dtype=torch.float64).expand(B, 4, 4).contiguous()
    dev = x.device
    T = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    its = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    corr = torch.empty(B, M, device=dev, dtype=torch.int32) if return_correspondence else None
    ws = torch.empty(_icp_workspace_bytes(B, M, N), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_icp_f32(px, py, pn, _vp(T0), r, _ICP_METHODS[method], max_iterations, relative_fitness, relative_rmse,
                                         _vp(T), _vp(fit), _vp(rmse), _vp(its), _vp(status), _vp(corr), _vp(ws), B, M, N, _KNN_FORMS[form],
                                         _stream()), "gecco_icp_f32")
    return ICPResult(*_unbatch([T, fit, rmse, its.long(), status.long(), None if corr is None else corr.long()], single))


def transform_points(points: Tensor, transform) -> Tensor:
    """A 4 x 4 transformation applied to a cloud: points (B, N, 3) or (N, 3), transform (4, 4) or (B, 4, 4), numbers or a tensor (what
    `icp` returns) -> R p + t in the dtype of `points`.  Plain torch on any device, differentiable in both arguments."""
    p, single = _cloud(points)
    T = transform if isinstance(transform, Tensor) else torch.as_tensor(transform, dtype=torch.float64)
    if T.is_complex() or tuple(T.shape) not in ((4, 4), (p.shape[0], 4, 4)) or (single and T.dim() != 2):
        raise ValueError(f"transform must be (4, 4){'' if single else f' or ({p.shape[0]}, 4, 4)'}")
    T = T.to(device=p.device, dtype=p.dtype)
    out = p @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]
    return out[0] if single else out


def fpfh(points: Tensor, normals: Tensor, k: int = 16, radius: float | None = None, idx: Tensor | None = None, return_spfh: bool = False,
         form: str | None = None):
    """FPFH descriptors of the points of a cloud from their k-neighbourhoods and normals (module docstring: the definition).  points and
    normals (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on fp32 contiguous copies); the normals are
    used as given (`estimate_normals(points)` or any others).  The search is `knn(points, points, k, exclude_self=False)` through `form`
    (None / "direct" / "split": same bits).  idx: the int64 or int32 (B, N, k) — (N, k) for single clouds — indices a caller already
    holds from that search (the ones `estimate_normals` takes); the search is skipped and k is idx's last dimension.  radius: only
    neighbours within it count.  Returns fpfh, fp32 (B, N, 33) or (N, 33); with return_spfh also spfh, fp32 of the same shape, and
    count, int64 (B, N).  ValueError for bad shapes, normals that do not match the points, k outside 1 .. KNN_MAX_K or above N, a radius
    that is not > 0, an idx whose shape disagrees with the clouds, mixed batched and single inputs, an unknown form; GeccoHipError for
    CPU tensors.  No gradient: the inputs are detached."""
    p, single = _cloud(points)
    if not isinstance(normals, Tensor):
        raise ValueError("normals must be a tensor")
    n, nsingle = _cloud(normals)
    if nsingle != single or n.shape != p.shape:
        raise ValueError(f"normals of shape {tuple(normals.shape)} do not belong to points of shape {tuple(points.shape)}")
    _check_form(form)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if idx is not None:
        if not isinstance(idx, Tensor) or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
            raise ValueError("idx must be an integer tensor")
        if idx.dim() != (2 if single else 3):
            raise ValueError("idx must be (N, k) for single clouds and (B, N, k) for batched ones")
        ix = idx[None] if single else idx
        if ix.shape[0] != B or ix.shape[1] != N:
            raise ValueError(f"idx of shape {tuple(idx.shape)} does not belong to {B} clouds of {N} points")
        k = ix.shape[2]
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k} is not in 1 .. {KNN_MAX_K}")
    if k > N:
        raise ValueError(f"k = {k} above the {N} points of a cloud")
    radius2 = 0.0   # no radius
    if radius is not None:
        try:
            radius = float(radius)
        except (TypeError, ValueError) as e:
            raise ValueError(f"radius = {radius!r} is not a number") from e
        if not radius > 0:
            raise ValueError(f"radius = {radius} must be > 0")
        radius2 = radius * radius   # rounded to fp32 on its way into the library
    x, px = _f32(p)
    y, py = _f32(n)
    if idx is None:
        ix, _ = _knn(x, x, k, False, False, form)
    else:
        if not ix.is_cuda:
            raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")
        ix = ix.detach().to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, N, FPFH_BINS, device=x.device, dtype=torch.float32)
    spfh = torch.empty(B, N, FPFH_BINS, device=x.device, dtype=torch.float32)
    cnt = torch.empty(B, N, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_fpfh_f32(px, py, _vp(ix), radius2, _vp(out), _vp(spfh), _vp(cnt), B, N, k, _stream()), "gecco_fpfh_f32")
    res = _unbatch([out, spfh, cnt.long()] if return_spfh else [out], single)
    return tuple(res) if return_spfh else res[0]


def _feature_nn_workspace_bytes(B: int, M: int, N: int) -> int:
    """GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N)"""
    return 8 * B * M * ((N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE)


def _feature_nn(a: Tensor, b: Tensor, want_d2: bool, form):
    """a (B, M, C), b (B, N, C) fp32 contiguous on the device -> idx (B, M) int32, d2 (B, M) fp32 or None"""
    B, M, Cn = a.shape
    N = b.shape[1]
    idx = torch.empty(B, M, device=a.device, dtype=torch.int32)
    d2 = torch.empty(B, M, device=a.device, dtype=torch.float32) if want_d2 else None
    # a workspace is offered where the auto rule can take the split form; the library decides (as in _knn)
    slices = (N + KNN_SPLIT_SLICE - 1) // KNN_SPLIT_SLICE
    offer = form == "split" or (form is None and slices > 1
                                and B * ((M + 63) // 64) < torch.cuda.get_device_properties(a.device).multi_processor_count)
    ws = torch.empty(_feature_nn_workspace_bytes(B, M, N), device=a.device, dtype=torch.uint8) if offer else None
    _lib.check(_lib.load().gecco_feature_nn_f32(_ptr(a), _ptr(b), _vp(idx), _ptr(d2), _vp(ws), B, M, N, Cn, _KNN_FORMS[form], _stream()),
               "gecco_feature_nn_f32")
    return idx, d2


def _features(t, name: str):
    if not isinstance(t, Tensor) or t.dim() not in (2, 3) or not t.is_floating_point():
        raise ValueError(f"{name}: expected floating features of shape (B, M, C) or (M, C)")
    single = t.dim() == 2
    return (t[None] if single else t), single


def match_features(source: Tensor, target: Tensor, mutual: bool = False, return_distances: bool = False, form: str | None = None):
    """The nearest row of `target` to every row of `source` in feature space (module docstring: the definition).  source (B, M, C) or
    (M, C), target (B, N, C) or (N, C) on the HIP device, 1 <= C <= FEATURE_MAX_DIM (what `fpfh` returns: C = 33), any float dtype and
    strides (computed on fp32 contiguous copies).  Returns corr, int64 (B, M) — (M,) for single sets — the index in `target` of each
    source row, equal distances going to the lowest index; with mutual, -1 where the match of that target row in `source` is not the
    row itself.  With return_distances also dist = sqrt(d2), fp32 of the same shape (the distance to the nearest row, also where
    `mutual` rejects it).  form None / "direct" / "split": the forms of `knn`, same bits either way.  ValueError for bad shapes, mixed
    batched and single inputs, mismatched batch sizes or channel counts, C outside 1 .. FEATURE_MAX_DIM, an unknown form; GeccoHipError
    for CPU tensors.  No gradient: indices (and the distances are detached)."""
    a, single = _features(source, "source")
    b, bsingle = _features(target, "target")
    if bsingle != single:
        raise ValueError("source and target must both be batched (B, ., C) or both single (., C)")
    if b.shape[0] != a.shape[0]:
        raise ValueError(f"source has {a.shape[0]} sets, target has {b.shape[0]}")
    if b.shape[2] != a.shape[2]:
        raise ValueError(f"source has {a.shape[2]} channels, target has {b.shape[2]}")
    _check_form(form)
    B, M, Cn = a.shape
    N = b.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or set")
    if not 1 <= Cn <= FEATURE_MAX_DIM:
        raise ValueError(f"C = {Cn} is not in 1 .. {FEATURE_MAX_DIM}")
    x, _ = _f32(a)
    y, _ = _f32(b)
    idx, d2 = _feature_nn(x, y, return_distances, form)
    corr = idx.long()
    if mutual:
        back, _ = _feature_nn(y, x, False, form)
        corr = torch.where(back.long().gather(1, corr) == torch.arange(M, device=corr.device)[None], corr, torch.full_like(corr, -1))
    out = [corr]
    if return_distances:
        out.append(d2.sqrt())
    out = _unbatch(out, single)
    return tuple(out) if return_distances else out[0]


class RANSACResult(NamedTuple):
    """What `ransac_registration` returns (module docstring: the definition).  status 0: found, 1: no surviving hypothesis with at
    least 3 inliers, 2: fewer than 3 pairs."""
    transformation: Tensor       # float64 (B, 4, 4): maps source onto target; the identity without a winner
    fitness: Tensor              # fp32 (B,): inliers / n_pairs under the final transformation
    inlier_rmse: Tensor          # fp32 (B,)
    n_pairs: Tensor              # int64 (B,): K, the usable correspondences
    best_hypothesis: Tensor      # int64 (B,): the winning h, -1 without one
    status: Tensor               # int64 (B,)
    inliers: Tensor | None       # int64 (B, M): correspondences[i] for the final inliers, -1 elsewhere
    hypotheses: tuple | None     # (triples int64 (B, H, 3), counts int64 (B, H): count or -code, sums float64 (B, H): +inf when rejected)


def _ransac_workspace_bytes(B: int, M: int, H: int) -> int:
    """GECCO_RANSAC_WORKSPACE_BYTES(B, M, H)"""
    return 32 * B * M + 16 * B * ((H + _RANSAC_BLOCK_HYPOTHESES - 1) // _RANSAC_BLOCK_HYPOTHESES) + 16 * B


def ransac_registration(source: Tensor, target: Tensor, correspondences: Tensor, max_correspondence_distance: float,
                        hypotheses: int | None = None, edge_similarity: float = 0.9, refine_passes: int = 1, seed: int = 0, candidates=None,
                        return_inliers: bool = False, return_hypotheses: bool = False) -> RANSACResult:
    """Global registration of `source` onto `target` by RANSAC on correspondences (module docstring: the definition): the `init` that
    `icp` needs, from what `match_features` returns.  source (B, M, 3) or (M, 3), target (B, N, 3) or (N, 3) on the HIP device, any float
    dtype and strides (computed on fp32 contiguous copies); correspondences (B, M) or (M,), any integer dtype: the target index of each
    source point, -1 (or anything outside [0, N)) for none.  hypotheses in 1 .. RANSAC_MAX_HYPOTHESES (default 100 000); edge_similarity
    in [0, 1], 0 switches the edge-length check off; refine_passes in 0 .. RANSAC_MAX_REFINE least-squares refits on the winner's inliers,
    always accepted (a polish of the consensus set, not a second search: the inlier count may fall by a borderline pair while the pose
    improves); seed in [0, 2^64), one for every cloud.  candidates: (H, 4, 4) or (B, H, 4, 4), numbers or a tensor: poses of your own to
    score instead of drawn ones (it sets H, so `hypotheses` must not be passed as well).  Returns a RANSACResult; for single clouds the
    batch dimension is dropped.  Three launches whatever the data and no synchronisation: the call can be captured in a hipGraph.
    ValueError, before any device call, for bad shapes, mixed batched and single inputs, mismatched batch sizes, correspondences that
    are not integers or not (B, M), a distance that is not a finite fp32 number > 0, hypotheses, refine_passes or seed that are not integers, those
    or edge_similarity out of range, candidates of the wrong shape or together with hypotheses; GeccoHipError for CPU tensors.  No gradient."""
    s, single = _cloud(source)
    t, tsingle = _cloud(target)
    _same_batching(s, single, t, tsingle, "source", "target")
    B, M, _ = s.shape
    N = t.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if not isinstance(correspondences, Tensor) or correspondences.is_floating_point() or correspondences.is_complex() or \
            correspondences.dtype == torch.bool:
        raise ValueError("correspondences must be an integer tensor")
    if tuple(correspondences.shape) != ((M,) if single else (B, M)):
        raise ValueError(f"correspondences of shape {tuple(correspondences.shape)} do not belong to a source of shape {tuple(source.shape)}")
    r = _positive_f32(max_correspondence_distance, "max_correspondence_distance", (TypeError, ValueError, OverflowError))
    try:
        edge_similarity = float(edge_similarity)
    except (TypeError, ValueError) as e:
        raise ValueError(f"edge_similarity = {edge_similarity!r} is not a number") from e
    if not 0.0 <= edge_similarity <= 1.0:
        raise ValueError(f"edge_similarity = {edge_similarity!r} is not in 0 .. 1")
    refine_passes, seed = _refits_and_seed(refine_passes, seed, RANSAC_MAX_REFINE)
    cand, H = _candidates_or_count(candidates, hypotheses, (4, 4), 100_000, RANSAC_MAX_HYPOTHESES, B, single)
    x, px = _f32(s)
    y, py = _f32(t)
    dev = x.device
    corr = correspondences.detach().reshape(B, M).to(device=dev)
    if corr.dtype != torch.int32:
        corr = corr.long().clamp(-1, N).int()   # widened first: narrow dtypes cannot hold N; wide indices outside [0, N) stay outside in 32 bits
    corr = corr.contiguous()
    if cand is not None:
        cand = cand.detach().to(device=dev, dtype=torch.float64).expand(B, H, 4, 4).contiguous()
    T = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    npairs = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    inl = torch.empty(B, M, device=dev, dtype=torch.int32) if return_inliers else None
    tri = torch.empty(B, H, 3, device=dev, dtype=torch.int32) if return_hypotheses else None
    cnt = torch.empty(B, H, device=dev, dtype=torch.int32) if return_hypotheses else None
    sums = torch.empty(B, H, device=dev, dtype=torch.float64) if return_hypotheses else None
    ws = torch.empty(_ransac_workspace_bytes(B, M, H), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_ransac_f32(px, py, _vp(corr), r, edge_similarity, H, refine_passes, seed, _vp(T), _vp(fit), _vp(rmse),
                                            _vp(npairs), _vp(best), _vp(status), _vp(inl), _vp(tri), _vp(cnt), _vp(sums), _vp(cand), _vp(ws),
                                            B, M, N, _stream()), "gecco_ransac_f32")
    out = _unbatch([T, fit, rmse, npairs.long(), best.long(), status.long(), None if inl is None else inl.long()], single)
    hyp = tuple(_unbatch([tri.long(), cnt.long(), sums], single)) if return_hypotheses else None
    return RANSACResult(*out, hyp)


class PlaneResult(NamedTuple):
    """What `segment_plane` returns (module docstring: the definition).  status 0: found, 1: no hypothesis reached the inlier bar,
    2: fewer than 3 usable points."""
    plane: Tensor                # float64 (B, 4): [a, b, c, d] with a unit normal, a x + b y + c z + d = 0; [0, 0, 1, 0] without a winner
    inliers: Tensor              # bool (B, N): the points within the threshold of the final plane
    n_inliers: Tensor            # int64 (B,)
    n_points: Tensor             # int64 (B,): K, the usable points
    best_hypothesis: Tensor      # int64 (B,): the winning h, -1 without one
    status: Tensor               # int64 (B,)
    fitness: Tensor              # fp32 (B,): n_inliers / n_points
    inlier_rmse: Tensor          # fp32 (B,)
    hypotheses: tuple | None     # (triples int64 (B, H, 3), planes fp32 (B, H, 6): the (nf, cf) scored, counts int64 (B, H): count or
                                 # -code, sums float64 (B, H): +inf when rejected)


class PlanesResult(NamedTuple):
    """What `segment_planes` returns: P = max_planes slots per cloud, the found ones first."""
    planes: Tensor               # float64 (B, P, 4): [0, 0, 1, 0] in a slot that found nothing
    labels: Tensor               # int64 (B, N): the slot whose plane took the point, -1 for none
    n_planes: Tensor             # int64 (B,): the slots with status 0, a prefix
    counts: Tensor               # int64 (B, P): the inliers of each slot
    status: Tensor               # int64 (B, P): the status of each slot's `segment_plane`


def _plane_workspace_bytes(B: int, N: int, H: int) -> int:
    """GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H)"""
    return 16 * B * N + 16 * B * ((H + _PLANE_BLOCK_HYPOTHESES - 1) // _PLANE_BLOCK_HYPOTHESES) + 16 * B


def _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers, viewpoint, candidates,
                     slots: int = 1):
    """The checks `segment_plane` and `segment_planes` share, all before any device call: the batched cloud, whether it was single, and
    the arguments as the library takes them (tensors still where the caller left them)."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    r = _positive_f32(distance_threshold, "distance_threshold", (TypeError, ValueError, OverflowError))
    refine_passes, seed = _refits_and_seed(refine_passes, seed, PLANE_MAX_REFINE, slots)
    min_inliers = _integer(min_inliers, "min_inliers")
    if not 0 <= min_inliers < 1 << 31:
        raise ValueError(f"min_inliers = {min_inliers} is not in 0 .. 2^31 - 1")
    if mask is not None:
        if not isinstance(mask, Tensor) or mask.is_floating_point() or mask.is_complex():
            raise ValueError("mask must be a bool or integer tensor")
        if tuple(mask.shape) != ((N,) if single else (B, N)):
            raise ValueError(f"mask of shape {tuple(mask.shape)} does not belong to points of shape {tuple(points.shape)}")
    if (axis is None) != (max_angle is None):
        raise ValueError("axis and max_angle must be given together")
    cos2 = 1.0
    if axis is not None:
        try:
            axis = _per_cloud_vector(axis, "axis", B, refuse_bool=True)
            max_angle = float(max_angle)
        except (TypeError, RuntimeError) as e:
            raise ValueError(f"axis must be (3,) or ({B}, 3) and max_angle = {max_angle!r} a number") from e
        if not 0.0 <= max_angle <= math.pi / 2:
            raise ValueError(f"max_angle = {max_angle!r} is not in 0 .. pi / 2 (radians)")
        cos2 = math.cos(max_angle) ** 2   # in double, on the host: part of the definition
    if viewpoint is not None:
        viewpoint = _per_cloud_vector(viewpoint, "viewpoint", B, refuse_bool=True)
    candidates, H = _candidates_or_count(candidates, hypotheses, (4,), 1024, PLANE_MAX_HYPOTHESES, B, single)
    return p, single, dict(r=r, H=H, refine_passes=refine_passes, seed=seed, mask=mask, axis=axis, cos2=cos2, min_inliers=min_inliers,
                           viewpoint=viewpoint, candidates=candidates)


def _plane_on_device(x: Tensor, a: dict) -> dict:
    """the tensor arguments as the library reads them, on the device of the fp32 cloud x (B, N, 3)"""
    B, N, _ = x.shape
    dev = x.device
    a = dict(a)
    if a["mask"] is not None:
        a["mask"] = (a["mask"].detach().to(device=dev).reshape(B, N) != 0).to(torch.uint8).contiguous()
    if a["axis"] is not None:
        a["axis"] = a["axis"].detach().to(device=dev, dtype=torch.float64).expand(B, 3).contiguous()
    if a["viewpoint"] is not None:
        a["viewpoint"] = a["viewpoint"].detach().to(device=dev, dtype=torch.float32).expand(B, 3).contiguous()
    if a["candidates"] is not None:
        a["candidates"] = a["candidates"].detach().to(device=dev, dtype=torch.float64).expand(B, a["H"], 4).contiguous()
    return a


def _plane_ransac(x: Tensor, px, a: dict, seed: int, mask, want_hyp: bool):
    """one gecco_plane_ransac_f32 on the fp32 contiguous cloud x (B, N, 3): the batched fields of a PlaneResult"""
    B, N, _ = x.shape
    H, dev = a["H"], x.device
    plane = torch.empty(B, 4, device=dev, dtype=torch.float64)
    fit = torch.empty(B, device=dev, dtype=torch.float32)
    rmse = torch.empty(B, device=dev, dtype=torch.float32)
    npts = torch.empty(B, device=dev, dtype=torch.int32)
    nin = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    inl = torch.empty(B, N, device=dev, dtype=torch.uint8)
    tri = torch.empty(B, H, 3, device=dev, dtype=torch.int32) if want_hyp else None
    hpl = torch.empty(B, H, 6, device=dev, dtype=torch.float32) if want_hyp else None
    cnt = torch.empty(B, H, device=dev, dtype=torch.int32) if want_hyp else None
    sums = torch.empty(B, H, device=dev, dtype=torch.float64) if want_hyp else None
    ws = torch.empty(_plane_workspace_bytes(B, N, H), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_plane_ransac_f32(px, _vp(mask), a["r"], H, a["refine_passes"], seed, _vp(a["axis"]), a["cos2"],
                                                  a["min_inliers"], _vp(a["viewpoint"]), _vp(a["candidates"]), _vp(plane), _vp(fit),
                                                  _vp(rmse), _vp(npts), _vp(nin), _vp(best), _vp(status), _vp(inl), _vp(tri), _vp(hpl),
                                                  _vp(cnt), _vp(sums), _vp(ws), B, N, _stream()), "gecco_plane_ransac_f32")
    hyp = (tri.long(), hpl, cnt.long(), sums) if want_hyp else None
    return [plane, inl.bool(), nin.long(), npts.long(), best.long(), status.long(), fit, rmse], hyp


def segment_plane(points: Tensor, distance_threshold: float, hypotheses: int | None = None, refine_passes: int = 1, seed: int = 0,
                  mask: Tensor | None = None, axis=None, max_angle: float | None = None, min_inliers: int = 3, viewpoint=None,
                  candidates=None, return_hypotheses: bool = False) -> PlaneResult:
    """The dominant plane of each cloud by RANSAC and the points on it (module docstring: the definition): Open3D's `segment_plane`,
    PCL's `SACSegmentation` with `SACMODEL_PLANE`, and with `axis` `SACMODEL_PERPENDICULAR_PLANE`.  points (B, N, 3) or (N, 3) on the HIP
    device, any float dtype and strides (computed on an fp32 contiguous copy); distance_threshold: a finite fp32 number > 0, the bound
    |t| <= r is inclusive; hypotheses in 1 .. PLANE_MAX_HYPOTHESES (default 1024); refine_passes in 0 .. PLANE_MAX_REFINE least-squares
    refits on the inliers, always accepted; seed in [0, 2^64), one for every cloud.  mask: bool or integer (B, N) or (N,), only points
    with a non-zero entry are drawn, scored or reported.  axis: (3,) or (B, 3), numbers or a tensor, with max_angle in radians in
    [0, pi / 2]: only planes whose normal is within max_angle of the axis, in either sense (a zero or non-finite axis constrains
    nothing); both or neither.  min_inliers: the winner needs max(3, min_inliers) inliers.  viewpoint: (3,) or (B, 3): the published
    normal points towards it.  candidates: (H, 4) or (B, H, 4), numbers or a tensor: planes [a, b, c, d] of your own to score instead
    of drawn ones (it sets H, so `hypotheses` must not be passed as well).  Returns a PlaneResult; for a single cloud the batch
    dimension is dropped.  Three launches whatever the data and no synchronisation: the call can be captured in a hipGraph.
    ValueError, before any device call, for bad shapes, a mask that is not bool / integer or of another shape, a threshold that is not a
    finite fp32 number > 0, hypotheses, refine_passes, seed or min_inliers that are not integers or out of range, axis without
    max_angle or the reverse, a max_angle outside [0, pi / 2], candidates of the wrong shape or together with hypotheses; GeccoHipError
    for CPU tensors.  No gradient."""
    p, single, a = _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers,
                                    viewpoint, candidates)
    x, px = _f32(p)
    a = _plane_on_device(x, a)
    out, hyp = _plane_ransac(x, px, a, a["seed"], a["mask"], return_hypotheses)
    return PlaneResult(*_unbatch(out, single), None if hyp is None else tuple(_unbatch(list(hyp), single)))


def segment_planes(points: Tensor, distance_threshold: float, max_planes: int, min_inliers: int, hypotheses: int | None = None,
                   refine_passes: int = 1, seed: int = 0, mask: Tensor | None = None, axis=None, max_angle: float | None = None,
                   viewpoint=None, candidates=None) -> PlanesResult:
    """Up to max_planes planes of each cloud, peeled one after another (PCL's loop of SACSegmentation + ExtractIndices): slot p is
    `segment_plane` with seed + p on the points no earlier slot took, mask & ~(inliers of the slots before), and needs min_inliers
    inliers.  Once a slot of a cloud finds nothing the cloud's mask is cleared, so the found slots are a prefix and the later ones
    report status 2.  The other arguments are `segment_plane`'s and serve every slot.  max_planes calls of the entry with torch
    elementwise operations between them and no synchronisation: 3 max_planes launches of the library, capturable in a hipGraph.
    Returns a PlanesResult: planes float64 (B, P, 4), labels int64 (B, N) with -1 for the points of no plane, n_planes int64 (B,),
    counts and status int64 (B, P); for a single cloud the batch dimension is dropped.  ValueError and GeccoHipError as `segment_plane`,
    and for a max_planes that is not an integer >= 1 or a seed whose last slot would pass 2^64 - 1.  No gradient."""
    P = _integer(max_planes, "max_planes")
    if P < 1:
        raise ValueError(f"max_planes = {P} must be >= 1")
    p, single, a = _plane_arguments(points, distance_threshold, hypotheses, refine_passes, seed, mask, axis, max_angle, min_inliers,
                                    viewpoint, candidates, slots=P)
    x, px = _f32(p)
    a = _plane_on_device(x, a)
    B, N, _ = x.shape
    free = torch.ones(B, N, device=x.device, dtype=torch.bool) if a["mask"] is None else a["mask"].bool()
    labels = torch.full((B, N), -1, device=x.device, dtype=torch.int64)
    planes, counts, status = [], [], []
    for slot in range(P):
        (plane, inl, nin, _, _, st, _, _), _ = _plane_ransac(x, px, a, a["seed"] + slot, free.to(torch.uint8), False)
        labels = torch.where(inl, slot, labels)
        free = free & ~inl & (st == 0)[:, None]
        planes.append(plane)
        counts.append(nin)
        status.append(st)
    status = torch.stack(status, 1)
    out = [torch.stack(planes, 1), labels, (status == 0).sum(1), torch.stack(counts, 1), status]
    return PlanesResult(*_unbatch(out, single))


def point_plane_distance(points: Tensor, plane) -> Tensor:
    """The signed distance n . p + d of every point from a plane [a, b, c, d] with a unit normal (what `segment_plane` returns): points
    (B, N, 3) or (N, 3), plane (4,) or (B, 4), numbers or a tensor -> (B, N) or (N,) in the dtype of `points`.  Plain torch on any
    device, differentiable in both arguments."""
    p, single = _cloud(points)
    q = plane if isinstance(plane, Tensor) else torch.as_tensor(plane, dtype=torch.float64)
    if q.is_complex() or tuple(q.shape) not in ((4,), (p.shape[0], 4)) or (single and q.dim() != 1):
        raise ValueError(f"plane must be (4,){'' if single else f' or ({p.shape[0]}, 4)'}")
    q = q.to(device=p.device, dtype=p.dtype)
    out = (p * q[..., None, :3]).sum(-1) + q[..., None, 3]
    return out[0] if single else out


class DBSCANResult(NamedTuple):
    """What `cluster_dbscan` returns (module docstring: the definition).  status 0: the fixed point was reached, 1: the round limit was
    hit and the labels describe a refinement of the true clusters."""
    labels: Tensor          # int64 (B, N): the cluster of each point, -1 for noise
    n_clusters: Tensor      # int64 (B,)
    core: Tensor            # bool (B, N): counts >= min_points
    status: Tensor          # int64 (B,)
    rounds: Tensor          # int64 (B,): hook + compress rounds run, the one that found the fixed point included
    counts: Tensor | None   # int64 (B, N): the neighbours of each point within eps, itself included


def _dbscan_workspace_bytes(B: int, N: int, R: int) -> int:
    """GECCO_DBSCAN_WORKSPACE_BYTES(B, N, R)"""
    return (4 * B * (5 * N + R) + 7) & ~7


def dbscan_default_rounds(N: int) -> int:
    """ceil(log2 max(N, 2)) + 2: the round limit `cluster_dbscan` takes by default, which no cloud of N points can exceed"""
    return (max(int(N), 2) - 1).bit_length() + 2


def cluster_dbscan(points: Tensor, eps: float, min_points: int = 10, max_rounds: int | None = None,
                   return_counts: bool = False) -> DBSCANResult:
    """DBSCAN clusters of each cloud (module docstring: the definition): Open3D's `cluster_dbscan`, scikit-learn's `DBSCAN`, and with
    min_points = 1 PCL's Euclidean cluster extraction, label for label.  points (B, N, 3) or (N, 3) on the HIP device, any float dtype
    and strides (computed on an fp32 contiguous copy); eps: the neighbourhood radius, a finite fp32 number > 0 whose square is one too
    (the bound dist2 <= fp32(eps * eps) is inclusive); min_points >= 1: the neighbours, itself included, that make a point a core
    point.  max_rounds in 0 .. DBSCAN_MAX_ROUNDS: the hook + compress rounds to launch; None takes ceil(log2 max(N, 2)) + 2, which
    cannot be exceeded, so status 1 only ever follows an explicit limit.  Returns a DBSCANResult: labels int64 (B, N) with -1 for noise,
    n_clusters int64 (B,), core bool (B, N), status and rounds int64 (B,), counts int64 (B, N) with return_counts and None without; for
    a single cloud the batch dimension is dropped.  The call makes 1 + 2 max_rounds + 2 launches and never synchronises: it can be
    captured in a hipGraph.  ValueError, before any device call, for bad shapes, an eps that is not a finite fp32 number > 0 with a
    finite square > 0, min_points or max_rounds that are not integers or out of range; GeccoHipError for CPU tensors.  No gradient:
    labels."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    e = _positive_f32(eps, "eps", (TypeError, ValueError, OverflowError))
    eps2 = C.c_float(e * e).value   # exact in double, rounded to fp32 once
    if not (math.isfinite(eps2) and eps2 > 0):
        raise ValueError(f"eps = {eps!r}: its square must be a finite fp32 number > 0")
    min_points = _integer(min_points, "min_points")
    if min_points < 1:
        raise ValueError(f"min_points = {min_points} must be >= 1")
    R = dbscan_default_rounds(N) if max_rounds is None else _integer(max_rounds, "max_rounds")
    if not 0 <= R <= DBSCAN_MAX_ROUNDS:
        raise ValueError(f"max_rounds = {R} is not in 0 .. {DBSCAN_MAX_ROUNDS}")
    x, px = _f32(p)
    dev = x.device
    labels = torch.empty(B, N, device=dev, dtype=torch.int32)
    ncl = torch.empty(B, device=dev, dtype=torch.int32)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)   # always: `core` comes from it
    rounds = torch.empty(B, device=dev, dtype=torch.int32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    ws = torch.empty(_dbscan_workspace_bytes(B, N, R), device=dev, dtype=torch.uint8)   # written by the library before it is read
    _lib.check(_lib.load().gecco_dbscan_f32(px, _vp(labels), _vp(ncl), _vp(cnt), _vp(rounds), _vp(status), _vp(ws), B, N, eps2, min_points,
                                            R, _stream()), "gecco_dbscan_f32")
    out = [labels.long(), ncl.long(), cnt >= min_points, status.long(), rounds.long(), cnt.long() if return_counts else None]
    return DBSCANResult(*_unbatch(out, single))


def cluster_sizes(labels: Tensor, n_clusters) -> Tensor:
    """The number of points of each cluster of `cluster_dbscan`: labels (B, N) or (N,), integers with -1 for noise -> int64 (B, C) or
    (C,), a `bincount` per cloud, which is what PCL's min / max cluster size filter needs.  n_clusters: C as an int (use it inside a
    graph), or the n_clusters tensor, which is read on the host (C = max(n_clusters.max(), 1)); columns at or after a cloud's own
    n_clusters are 0, labels outside [0, C) are skipped.  Plain torch on any device."""
    if not isinstance(labels, Tensor) or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool or \
            labels.dim() not in (1, 2):
        raise ValueError("labels must be an integer tensor of shape (B, N) or (N,)")
    single = labels.dim() == 1
    lab = (labels[None] if single else labels).long()
    Cn = max(int(n_clusters.max()), 1) if isinstance(n_clusters, Tensor) else _integer(n_clusters, "n_clusters")
    if Cn < 1:
        raise ValueError(f"n_clusters = {Cn} must be >= 1")
    B = lab.shape[0]
    rows = torch.where((lab >= 0) & (lab < Cn), lab, Cn) + (Cn + 1) * torch.arange(B, device=lab.device)[:, None]   # column C: skipped
    out = torch.bincount(rows.reshape(-1), minlength=B * (Cn + 1)).view(B, Cn + 1)[:, :Cn]
    return out[0] if single else out


class RadiusNeighbors(NamedTuple):
    """What `radius_search` returns without max_neighbors (module docstring: the definition): the neighbour lists of every query in
    CSR form.  Row r = b * M + i, query i of cloud b, owns the entries [row_splits[r], row_splits[r + 1])."""
    indices: Tensor            # int64 (nnz,): j in [0, N) of the row's own cloud
    row_splits: Tensor         # int64 (B * M + 1,)
    distances: Tensor | None   # fp32 (nnz,): sqrt(dist2)
    counts: Tensor             # int64 (B, M): row_splits[r + 1] - row_splits[r]


def _radius_f32(radius):
    """A radius as the library takes it -> (the radius rounded to fp32, r2 = fp32(radius * radius)); ValueError unless both are finite
    numbers > 0"""
    rad = _positive_f32(radius, "radius", (TypeError, ValueError, OverflowError))
    r2 = C.c_float(rad * rad).value   # exact in double, rounded to fp32 once
    if not (math.isfinite(r2) and r2 > 0):
        raise ValueError(f"radius = {radius!r}: its square must be a finite fp32 number > 0")
    return rad, r2


def _radius_arguments(query: Tensor, ref: Tensor | None, radius, exclude_self):
    """What the three radius operators check before any device call -> q (B, M, 3), r (B, N, 3) or None (= q), single, N,
    r2 = fp32(radius * radius) and exclude_self as a bool"""
    q, single = _cloud(query)
    r = None
    if ref is not None:
        r, rsingle = _cloud(ref)
        _same_batching(q, single, r, rsingle, "query", "ref")
    B, M, _ = q.shape
    N = M if r is None else r.shape[1]
    if B < 1 or M < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    exclude_self = (ref is None) if exclude_self is None else bool(exclude_self)
    if exclude_self and M != N:
        raise ValueError(f"exclude_self needs the query cloud to be the reference cloud (M = {M}, N = {N})")
    return q, r, single, N, _radius_f32(radius)[1], exclude_self


def _radius_inputs(q: Tensor, r: Tensor | None):
    """the fp32 contiguous copies of both clouds (one copy when they are the same cloud) and their pointers"""
    x, px = _f32(q)
    y, py = (x, px) if r is None or r is q else _f32(r)
    return x, px, y, py


def _radius_counts(x: Tensor, px, py, N: int, r2: float, exclude_self: bool) -> Tensor:
    """the count launch: int32 (B, M)"""
    B, M, _ = x.shape
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_radius_count_f32(px, py, _vp(cnt), B, M, N, r2, int(exclude_self), _stream()), "gecco_radius_count_f32")
    return cnt


class GridIndex(NamedTuple):
    """What `build_grid_index` returns (module docstring: the definition): a cloud sorted into the cells of a uniform grid, for
    `radius_count`, `radius_search` and `radius_outlier_mask` with `index=`.  Position s of the sorted order holds point perm[s]; the
    on-grid points come first, by (cell key, original index), the off-grid points last."""
    points: Tensor          # fp32 (B, N, 3): the copy the index was built from, the reference cloud of every query
    sorted_points: Tensor   # fp32 (B, N, 4): (x, y, z, the bits of perm) per sorted position
    perm: Tensor            # int32 (B, N)
    keys: Tensor            # int64 (B, N): the sorted cell keys; an off-grid point's is -2^63 (bit 63 alone)
    table_keys: Tensor      # int64 (B, cap): the open-addressing table, cap = the power of two >= 2 N; -1 = empty
    table_range: Tensor     # int32 (B, cap, 2): the run [start, end) of the slot's key in the sorted order
    n_in_grid: Tensor       # int32 (B,): the number of on-grid points
    origin: Tensor          # fp32 (B, 3)
    cell_size: float        # as rounded to fp32
    single: bool            # built from an (N, 3) cloud


_INT64_MIN = -(1 << 63)


def _grid_cell_size(cell_size) -> float:
    size = _positive_f32(cell_size, "cell_size", (TypeError, ValueError, OverflowError))
    if not math.isfinite(C.c_float(1.0 / size).value):
        raise ValueError(f"cell_size = {cell_size!r}: its reciprocal must be a finite fp32 number")
    return size


def _grid_sorted_keys(x: Tensor, px, origin: Tensor, size: float):
    """the key launch and the sort: the keys of x (B, N, 3) in the grid (origin, size), sorted as unsigned integers (int64 sorts signed:
    key ^ 2^63 has that order), and the int64 permutation"""
    B, N, _ = x.shape
    keys = torch.empty(B, N, device=x.device, dtype=torch.int64)
    _lib.check(_lib.load().gecco_grid_keys_f32(px, _ptr(origin), size, _vp(keys), B, N, _stream()), "gecco_grid_keys_f32")
    flipped, order = torch.sort(keys ^ _INT64_MIN, dim=1, stable=True)   # stable: a cell's points ascend in original index
    return flipped ^ _INT64_MIN, order


def _grid_build(x: Tensor, px, size: float, org, single: bool) -> GridIndex:
    """x: the fp32 contiguous cloud (B, N, 3) on the device; org: None or what `_per_cloud_vector` accepted"""
    B, N, _ = x.shape
    dev = x.device
    origin = (torch.zeros(B, 3, device=dev, dtype=torch.float32) if org is None
              else org.detach().to(device=dev, dtype=torch.float32).expand(B, 3).contiguous())
    keys, order = _grid_sorted_keys(x, px, origin, size)
    perm = order.to(torch.int32)
    cap = 1 << (2 * N - 1).bit_length()   # GECCO_GRID_CAPACITY(N)
    sorted_points = torch.empty(B, N, 4, device=dev, dtype=torch.float32)
    table_keys = torch.empty(B, cap, device=dev, dtype=torch.int64)       # filled by the library, inside the call
    table_range = torch.empty(B, cap, 2, device=dev, dtype=torch.int32)
    n_in_grid = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().gecco_grid_build_f32(px, _vp(keys), _vp(perm), _vp(sorted_points), _vp(table_keys), _vp(table_range),
                                                _vp(n_in_grid), B, N, _stream()), "gecco_grid_build_f32")
    return GridIndex(x, sorted_points, perm, keys, table_keys, table_range, n_in_grid, origin, size, single)


def build_grid_index(points: Tensor, cell_size: float, origin=None) -> GridIndex:
    """A uniform-grid index over `points` for the fixed-radius operators (module docstring: the definition): build it once, then pass
    `index=` to `radius_count`, `radius_search` or `radius_outlier_mask` at any radius <= cell_size; each query then tests the points
    of the at most 4 x 4 x 4 cells its ball can reach instead of the whole cloud.  points (B, N, 3) or (N, 3) on the HIP device, any
    float dtype and strides (computed on the fp32 contiguous copy, which the index keeps); cell_size a finite fp32 number > 0 with a
    finite reciprocal; origin (3,) or (B, 3), numbers or a tensor, as in `voxel_downsample` (default 0).  A point's cell is
    `voxel_downsample`'s for voxel_size = cell_size; the points that filter would drop stay in the index as its tail and are found
    like any other.  A key launch, a stable torch.sort of the int64 keys, a table fill and a build launch: no host synchronisation.
    ValueError, before any device call, for bad shapes, a bad cell_size, an origin of the wrong shape; GeccoHipError for CPU tensors.
    Not under graph capture (the sort allocates): build outside, query inside."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    size = _grid_cell_size(cell_size)
    org = None if origin is None else _per_cloud_vector(origin, "origin", B, refuse_bool=True)
    x, px = _f32(p)
    return _grid_build(x, px, size, org, single)


def _grid_arguments(query: Tensor, ref: Tensor | None, radius, exclude_self, index):
    """What the radius operators check before any device call when `index` is given -> q (B, M, 3), single, r2, exclude_self, and
    either the GridIndex to query or, for index="grid", the reference cloud to build one over (None: q itself) with the cell size"""
    if isinstance(index, GridIndex):
        if ref is not None:
            raise ValueError("with a GridIndex the reference cloud is index.points: ref must be None")
        q, single = _cloud(query)
        _same_batching(q, single, index.points, index.single, "query", "index")
        B, M, _ = q.shape
        N = index.points.shape[1]
        if B < 1 or M < 1:
            raise ValueError("empty batch or cloud")
        exclude_self = bool(exclude_self) if exclude_self is not None else False
        if exclude_self and M != N:
            raise ValueError(f"exclude_self needs the query cloud to be the reference cloud (M = {M}, N = {N})")
        rad, r2 = _radius_f32(radius)
        if rad > index.cell_size:
            raise ValueError(f"radius = {rad} is above the index's cell_size = {index.cell_size}: build an index with a larger cell")
        return q, single, r2, exclude_self, index, None, None
    if not (isinstance(index, str) and index == "grid"):
        raise ValueError("index must be None, 'grid' or a GridIndex")
    q, r, single, _, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
    if r is not None and r.shape[1] > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {r.shape[1]} above {VOXEL_MAX_POINTS}")
    return q, single, r2, exclude_self, None, r, _grid_cell_size(_radius_f32(radius)[0])


def _grid_inputs(q: Tensor, exclude_self: bool, index, r, size):
    """the device side of `_grid_arguments`: the fp32 queries, the index (built here for index="grid") and the order the queries are
    answered in: the index's own when the queries are its cloud, else that of their own cell keys"""
    x, px = _f32(q)
    same = index is None and (r is None or r is q)
    if index is None:
        y, py = (x, px) if same else _f32(r)
        index = _grid_build(y, py, size, None, False)
    if same or exclude_self:
        qorder = index.perm
    else:
        qorder = _grid_sorted_keys(x, px, index.origin, index.cell_size)[1].to(torch.int32)
    return x, px, index, qorder


def _grid_counts(x: Tensor, px, g: GridIndex, qorder: Tensor, r2: float, exclude_self: bool) -> Tensor:
    """the count launch on an index: int32 (B, M)"""
    B, M, _ = x.shape
    cnt = torch.empty(B, M, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().gecco_grid_radius_count_f32(px, _vp(qorder), _vp(g.sorted_points), _vp(g.table_keys), _vp(g.table_range),
                                                       _vp(g.n_in_grid), _vp(g.origin), g.cell_size, _vp(cnt), B, M, g.points.shape[1], r2,
                                                       int(exclude_self), _stream()), "gecco_grid_radius_count_f32")
    return cnt


def radius_count(query: Tensor, ref: Tensor | None = None, radius: float | None = None, exclude_self: bool | None = None,
                 index=None) -> Tensor:
    """The number of points of `ref` within `radius` of every point of `query` (module docstring: the definition; the bound
    dist2 <= fp32(radius * radius) is inclusive).  query (B, M, 3) or (M, 3), ref (B, N, 3) or (N, 3) on the HIP device, any float dtype
    and strides (computed on fp32 contiguous copies).  ref=None: the query cloud itself, and exclude_self then defaults to True (a point
    does not count itself); with a ref it defaults to False.  Returns int64 (B, M), (M,) for a single cloud, never clamped.  One launch,
    no synchronisation: the call can be captured in a hipGraph.  ValueError, before any device call, for bad shapes, mixed batching, a
    radius that is not a finite fp32 number > 0 with a finite square > 0, exclude_self with M != N; GeccoHipError for CPU tensors.  No
    gradient: counts.

    index=None: the direct scan of the whole reference cloud.  index=a GridIndex (`build_grid_index`): the same counts from the cells
    within reach; the reference cloud is index.points, so ref must be None, exclude_self defaults to False and, when set, means that
    the queries ARE the index's cloud (M == N); radius <= index.cell_size.  One launch (and, for queries that are not the index's
    cloud, a key launch and a sort for the order they are answered in); against a prebuilt index in self mode the call can be captured.
    index="grid": builds an index over the reference cloud with cell_size = radius for this call; ref and exclude_self as without.
    Further ValueErrors: ref with a GridIndex, an index of another batch, a radius above the cell size, an unknown index."""
    if index is not None:
        q, single, r2, exclude_self, g, r, size = _grid_arguments(query, ref, radius, exclude_self, index)
        x, px, g, qorder = _grid_inputs(q, exclude_self, g, r, size)
        cnt = _grid_counts(x, px, g, qorder, r2, exclude_self).long()
        return cnt[0] if single else cnt
    q, r, single, N, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
    x, px, _, py = _radius_inputs(q, r)
    cnt = _radius_counts(x, px, py, N, r2, exclude_self).long()
    return cnt[0] if single else cnt


def _grid_radius_search(query, ref, radius, exclude_self, max_neighbors, order, return_distances, index) -> RadiusNeighbors:
    """`radius_search` with an index: the CSR form, filled in the order of the index and sorted into the order asked for"""
    q, single, r2, exclude_self, g, r, size = _grid_arguments(query, ref, radius, exclude_self, index)
    if order not in ("index", "distance", "grid"):
        raise ValueError("order must be 'index', 'distance' or 'grid'")
    if max_neighbors is not None:
        raise ValueError("max_neighbors cannot be combined with index: the fixed-width forms run on the direct scan")
    x, px, g, qorder = _grid_inputs(q, exclude_self, g, r, size)
    B, M, _ = x.shape
    dev, rows = x.device, B * M
    want_d2 = return_distances or order == "distance"
    cnt = _grid_counts(x, px, g, qorder, r2, exclude_self)
    splits = torch.zeros(rows + 1, device=dev, dtype=torch.int64)
    torch.cumsum(cnt.view(-1), 0, dtype=torch.int64, out=splits[1:])
    nnz = int(splits[-1])   # the one synchronisation
    idx = torch.empty(nnz, device=dev, dtype=torch.int32)
    d2 = torch.empty(nnz, device=dev, dtype=torch.float32) if want_d2 else None
    if nnz:
        _lib.check(_lib.load().gecco_grid_radius_search_f32(px, _vp(qorder), _vp(g.sorted_points), _vp(g.table_keys), _vp(g.table_range),
                                                            _vp(g.n_in_grid), _vp(g.origin), g.cell_size, _vp(splits), _vp(idx), _ptr(d2), B, M,
                                                            g.points.shape[1], r2, int(exclude_self), _stream()),
                   "gecco_grid_radius_search_f32")
        if order != "grid":
            row = torch.repeat_interleave(torch.arange(rows, device=dev), cnt.view(-1).long(), output_size=nnz) << 32
            perm = torch.sort(row | idx.long()).indices   # (row, j) is unique: ascending j inside every row
            if order == "distance":   # stable: equal (row, dist2) keep their ascending j
                perm = perm[torch.sort(row | d2[perm].view(torch.int32).long(), stable=True).indices]
            idx, d2 = idx[perm], None if d2 is None else d2[perm]
    counts = cnt.long()
    return RadiusNeighbors(idx.long(), splits, d2.sqrt() if return_distances else None, counts[0] if single else counts)


def radius_search(query: Tensor, ref: Tensor | None = None, radius: float | None = None, exclude_self: bool | None = None,
                  max_neighbors: int | None = None, order: str = "index", return_distances: bool = True, index=None):
    """Every point of `ref` within `radius` of every point of `query` (module docstring: the definition).  Clouds, radius and
    exclude_self as in `radius_count`.  order "index": a row's neighbours in ascending j; "distance": by (dist2, j) ascending, `knn`'s
    order.

    index (a GridIndex or "grid", as in `radius_count`): the same RadiusNeighbors from the cells within reach, element for element and
    bit for bit, by count -> cumsum -> one host read -> fill on the index.  The fill leaves a row in the order of the index; order
    "index" is then one torch.sort of (row << 32 | j) over the entries, "distance" that sort followed by the stable sort below, and
    order "grid", accepted only with an index, returns the rows as filled: ascending position in the index's sorted order, that is by
    (cell key, j) with the off-grid points last.  It is deterministic, costs no sort and suits consumers that pool over a
    neighbourhood.  max_neighbors together with index is a ValueError: the fixed-width forms stay on the direct scan (a follow-up).

    max_neighbors=None (Open3D's search_radius_vector_3d): a RadiusNeighbors in CSR form, indices int64 (nnz,), row_splits int64
    (B * M + 1,), distances = sqrt(dist2) fp32 (nnz,) (None without return_distances) and counts int64 (B, M), (M,) for a single cloud.
    A count launch, an int64 cumsum on the device, ONE host read of the total to size the outputs (the call's only synchronisation)
    and a fill launch, none when nothing is within the radius.  The distance order is a stable sort of the index-ordered entries by
    (row, dist2's bits), in torch.

    max_neighbors=K: (idx int64 (B, M, K) padded with -1, dist fp32 padded with +inf or None without return_distances, counts int64
    (B, M), unclamped); the batch dimension is dropped for single clouds.  No synchronisation: the call can be captured in a hipGraph.
    order "index", 1 <= K <= N: the FIRST K neighbours by index, one launch (PointNet++'s ball query).  order "distance", 1 <= K <=
    min(KNN_MAX_K, candidates of a query): the K NEAREST, cut at the radius (Open3D's search_hybrid_vector_3d): `knn`, the count
    launch and a mask on dist2 <= r2.

    ValueError, before any device call, for what `radius_count` refuses, an unknown order, max_neighbors that is not an integer or out
    of range; GeccoHipError for CPU tensors.  No gradient: indices (and the distances are detached)."""
    if index is not None:
        return _grid_radius_search(query, ref, radius, exclude_self, max_neighbors, order, return_distances, index)
    q, r, single, N, r2, exclude_self = _radius_arguments(query, ref, radius, exclude_self)
    if order not in ("index", "distance"):
        raise ValueError("order must be 'index' or 'distance'" + (" ('grid' needs an index)" if order == "grid" else ""))
    B, M, _ = q.shape
    K = None
    if max_neighbors is not None:
        K = _integer(max_neighbors, "max_neighbors")
        limit = N if order == "index" else min(KNN_MAX_K, N - int(exclude_self))
        if not 1 <= K <= limit:
            raise ValueError(f"max_neighbors = {K} is not in 1 .. {limit}" + (" (order 'distance': KNN_MAX_K and the candidates of a query)"
                                                                             if order == "distance" else " (N)"))
    x, px, y, py = _radius_inputs(q, r)
    dev, lib, null = x.device, _lib.load(), C.c_void_p(0)
    want_d2 = return_distances or (K is None and order == "distance")

    if K is not None and order == "distance":   # the hybrid search: the k nearest, cut at the radius
        idx, d2 = _knn(x, None if y is x else y, K, exclude_self, True, None)
        cnt = _radius_counts(x, px, py, N, r2, exclude_self)
        inside = d2 <= r2   # (dist2 >= 0 or +inf: the float order is the order of the bits)
        out = [idx.long().masked_fill(~inside, -1), d2.sqrt().masked_fill(~inside, math.inf) if return_distances else None, cnt.long()]
        return tuple(_unbatch(out, single))

    if K is not None:   # the first K by index: one launch
        idx = torch.empty(B, M, K, device=dev, dtype=torch.int32)
        d2 = torch.empty(B, M, K, device=dev, dtype=torch.float32) if want_d2 else None
        cnt = torch.empty(B, M, device=dev, dtype=torch.int32)
        _lib.check(lib.gecco_radius_search_f32(px, py, null, _vp(idx), _ptr(d2), _vp(cnt), B, M, N, r2, int(exclude_self), K, _stream()),
                   "gecco_radius_search_f32")
        return tuple(_unbatch([idx.long(), d2.sqrt() if return_distances else None, cnt.long()], single))

    cnt = _radius_counts(x, px, py, N, r2, exclude_self)
    rows = B * M
    splits = torch.zeros(rows + 1, device=dev, dtype=torch.int64)
    torch.cumsum(cnt.view(-1), 0, dtype=torch.int64, out=splits[1:])   # exact; splits[:rows] is the exclusive prefix sum
    nnz = int(splits[-1])   # the one synchronisation
    idx = torch.empty(nnz, device=dev, dtype=torch.int32)
    d2 = torch.empty(nnz, device=dev, dtype=torch.float32) if want_d2 else None
    if nnz:
        _lib.check(lib.gecco_radius_search_f32(px, py, _vp(splits), _vp(idx), _ptr(d2), null, B, M, N, r2, int(exclude_self), 0, _stream()),
                   "gecco_radius_search_f32")
        if order == "distance":   # stable: equal (row, dist2) keep their ascending j
            row = torch.repeat_interleave(torch.arange(rows, device=dev), cnt.view(-1).long(), output_size=nnz)
            perm = torch.sort((row << 32) | d2.view(torch.int32).long(), stable=True).indices
            idx, d2 = idx[perm], d2[perm]
    counts = cnt.long()
    return RadiusNeighbors(idx.long(), splits, d2.sqrt() if return_distances else None, counts[0] if single else counts)


def radius_outlier_mask(points: Tensor, radius: float, min_neighbors: int, return_counts: bool = False, index=None):
    """The radius outlier filter of Open3D (`remove_radius_outlier`) and PCL (`RadiusOutlierRemoval`) on `radius_count`: keep_i =
    count_i >= min_neighbors with count_i the points within `radius` of point i, itself excluded (Open3D's `indices.size() > nb_points`
    counts the point among its own results).  points (B, N, 3) or (N, 3) -> a bool mask (B, N) or (N,), True for the points to keep;
    with return_counts also the int64 counts of the same shape.  min_neighbors: an integer >= 0.  One launch, no synchronisation.
    index: as in `radius_count` ("grid", or a GridIndex built over these points): the same mask from the grid."""
    min_neighbors = _integer(min_neighbors, "min_neighbors")
    if min_neighbors < 0:
        raise ValueError(f"min_neighbors = {min_neighbors} must be >= 0")
    counts = radius_count(points, None, radius, True, index=index)
    keep = counts >= min_neighbors
    return (keep, counts) if return_counts else keep


class ISSResult(NamedTuple):
    """What `iss_keypoints` returns (module docstring: the definition); the batch dimension is dropped for a single cloud"""
    mask: Tensor          # bool (B, N): True for a keypoint
    saliency: Tensor      # fp64 (B, N): lambda0 of a candidate, 0 otherwise
    eigenvalues: Tensor   # fp64 (B, N, 3): ascending; 0 where the salient ball holds fewer than min_neighbors or only identical points
    counts: Tensor        # int64 (B, N): the points of the salient ball, the point itself among them
    n_keypoints: Tensor   # int64 (B,): the row sums of the mask


def _gamma(value, name: str) -> float:
    try:
        if isinstance(value, bool):
            raise TypeError
        v = float(value)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"{name} = {value!r} is not a number") from e
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} = {value!r} must be a finite number > 0")
    return v


def iss_keypoints(points: Tensor, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                  min_neighbors: int = 5, index: GridIndex | None = None) -> ISSResult:
    """The ISS keypoints of every cloud (module docstring: the definition): Open3D's `compute_iss_keypoints`, PCL's `ISSKeypoint3D`.
    points (B, N, 3) or (N, 3) on the HIP device, any float dtype and strides (computed on the fp32 contiguous copy).  salient_radius:
    the ball the scatter matrix of a point is pooled over; non_max_radius: the ball a keypoint's saliency must be the largest of; both
    plain numbers shared by the batch, as `radius_count` takes them (Open3D's defaults are 6 x and 4 x `cloud_resolution`).  gamma_21,
    gamma_32: the bounds on lambda1 / lambda2 and lambda0 / lambda1, finite numbers > 0; min_neighbors: an integer >= 1, the least
    number of points (the point itself counts) in either ball.  Returns an ISSResult; index the cloud, or the rows of `fpfh`, with
    its mask.
    index=None builds a grid index for the call with cell_size = max(salient_radius, non_max_radius) and origin 0 (the sort of the
    build allocates, as `build_grid_index` documents).  index=a GridIndex built over THESE points (`build_grid_index`; its cell_size >=
    both radii) is reused: the call is then two launches with no allocation inside the library and no host synchronisation, and can
    be captured in a graph.  The same parameters give the same bits either way; an index with another cell or origin gives the same
    counts and may differ in the last bits of the eigenvalues.  The grid is the only form: there is no direct scan.
    ValueError, before any device call, for bad shapes or an empty cloud, N above VOXEL_MAX_POINTS, a radius that is not a finite
    fp32 number > 0 with a finite square > 0, a gamma that is not a finite number > 0, min_neighbors that is not an integer >= 1,
    an index that is neither None nor a GridIndex, an index of another batching or another N, a radius above the index's cell;
    GeccoHipError for CPU tensors.  No gradient: a selection."""
    p, single = _cloud(points)
    B, N, _ = p.shape
    if B < 1 or N < 1:
        raise ValueError("empty batch or cloud")
    (rs, r2s), (rn, r2n) = _radius_f32(salient_radius), _radius_f32(non_max_radius)
    if N > VOXEL_MAX_POINTS:
        raise ValueError(f"N = {N} above {VOXEL_MAX_POINTS}")
    g21, g32 = _gamma(gamma_21, "gamma_21"), _gamma(gamma_32, "gamma_32")
    min_neighbors = _integer(min_neighbors, "min_neighbors")
    if not 1 <= min_neighbors <= 0x7fffffff:
        raise ValueError(f"min_neighbors = {min_neighbors} must be in 1 .. 2^31 - 1")
    if index is None:
        size = _grid_cell_size(max(rs, rn))
    elif isinstance(index, GridIndex):
        _same_batching(p, single, index.points, index.single, "points", "index")
        if index.points.shape[1] != N:
            raise ValueError(f"points has {N} points a cloud, the index was built over {index.points.shape[1]}")
        size = index.cell_size
    else:
        raise ValueError("index must be None or a GridIndex")
    cell2 = C.c_float(size * size).value   # the library's fp32 product
    for name, r2 in (("salient_radius", r2s), ("non_max_radius", r2n)):
        if not r2 <= cell2:
            raise ValueError(f"{name}: its square {r2} is above the square of the index's cell_size = {size}: build an index with a larger cell")
    if index is None:
        x, px = _f32(p)
        index = _grid_build(x, px, size, None, single)
    elif not (p.is_cuda and index.sorted_points.is_cuda):
        raise _lib.GeccoHipError("gecco_amd operators need tensors on the HIP device (no CPU fallback)")
    dev = index.sorted_points.device
    saliency = torch.empty(B, N, device=dev, dtype=torch.float64)
    eig = torch.empty(B, N, 3, device=dev, dtype=torch.float64)
    cnt = torch.empty(B, N, device=dev, dtype=torch.int32)
    mask = torch.empty(B, N, device=dev, dtype=torch.bool)
    _lib.check(_lib.load().gecco_iss_keypoints_f32(_vp(index.sorted_points), _vp(index.table_keys), _vp(index.table_range), _vp(index.n_in_grid),
                                                   _vp(index.origin), index.cell_size, _vp(saliency), _vp(eig), _vp(cnt), _vp(mask), B, N, r2s,
                                                   r2n, g21, g32, min_neighbors, _stream()), "gecco_iss_keypoints_f32")
    return ISSResult(*_unbatch([mask, saliency, eig, cnt.long(), mask.sum(1)], single))


def cloud_resolution(points: Tensor) -> Tensor:
    """Open3D's `ComputeModelResolution`: per cloud, the mean distance of a point to the nearest OTHER point, fp64 (B,) — a 0-d tensor
    for a single cloud.  `knn` with k = 1 in self mode, sqrt of its fp32 dist2, summed in fp64 over the finite entries (a non-finite
    point has none and is nobody's nearest while a finite point remains); 0 for a cloud without a finite entry.  Plain torch on the
    search.  Open3D's default radii for `iss_keypoints` are 6 x and 4 x this number.  ValueError for bad shapes and clouds of fewer
    than 2 points; GeccoHipError for CPU tensors."""
    p, single = _cloud(points)
    _, d2 = _knn(p, None, 1, True, True, None)
    d = d2[:, :, 0].sqrt()
    finite = torch.isfinite(d)
    total = torch.where(finite, d, torch.zeros_like(d)).double().sum(1)
    n = finite.sum(1)
    out = torch.where(n > 0, total / n.clamp(min=1), torch.zeros_like(total))
    return out[0] if single else out
