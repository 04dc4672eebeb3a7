// tvr_mesh_api.hip — the tvr_mesh_* entry points of libtvr.so (include/tvr.h), all but tvr_mesh_project (it reads a scene: tvr_api.hip).  Host code only and no kernel:
// argument checks, scratch carving and the launchers of tvr_mesh*.hip on the caller's stream.  Every check precedes the first launch, and a call's checks run in a
// fixed order: the first one that fails decides the status and the text of tvr_last_error().
#include "tvr_kernels.h"
#include "tvr_host.h"

// ---- the checks that recur ------------------------------------------------------------------------------------------------------------------------------------------
// a scratch buffer, blob or table: not NULL, 256-byte aligned, at least `want` bytes (`query` is the size query the caller should have asked).  A short buffer is
// `short_code`: TVR_ERR_INVALID in the calls up to the smoothing, TVR_ERR_SCRATCH from the rasteriser on
static int buffer_check(const char *fn, const char *what, const void *p, size_t have, size_t want, const char *query, int short_code)
{
    if (!p) return fail(TVR_ERR_INVALID, "%s: %s is NULL", fn, what);
    if ((uintptr_t)p % 256) return fail(TVR_ERR_INVALID, "%s: %s is not 256-byte aligned", fn, what);
    if (have < want) return fail(short_code, "%s: %s holds %zu B, %s asks for %zu B", fn, what, have, query, want);
    return TVR_OK;
}

// a count `name` = n: not negative, at most `max` (`why` ends the sentence).  Where other checks stand between the two, the first call passes INT64_MAX
static int count_check(const char *fn, const char *name, int64_t n, int64_t max, const char *why)
{
    if (n < 0) return fail(TVR_ERR_INVALID, "%s: %s = %lld is negative", fn, name, (long long)n);
    if (n > max) return fail(TVR_ERR_UNSUPPORTED, "%s: %s = %lld: %s", fn, name, (long long)n, why);
    return TVR_OK;
}

// the vertex count and a second count (`other`: n_triangles or n_half_edges), reported together
static int pair_counts(const char *fn, int64_t n_vertices, const char *other, int64_t n_other, int64_t max_other, const char *why)
{
    if (n_vertices < 0 || n_other < 0) return fail(TVR_ERR_INVALID, "%s: n_vertices %lld / %s %lld is negative", fn, (long long)n_vertices, other, (long long)n_other);
    if (n_vertices > INT32_MAX || n_other > max_other)
        return fail(TVR_ERR_UNSUPPORTED, "%s: n_vertices %lld / %s %lld: %s", fn, (long long)n_vertices, other, (long long)n_other, why);
    return TVR_OK;
}

// an output of n (+ `plus`) rows of `row_bytes` each; `unit` names rows and row, as in "vertices x 3 fp32"
static int out_check(const char *fn, const char *what, size_t have, int64_t n, int plus, size_t row_bytes, const char *unit, int code)
{
    const size_t want = ((size_t)n + plus) * row_bytes;
    if (have < want) return fail(code, "%s: %s holds %zu B, %lld %s need %zu B", fn, what, have, (long long)n, unit, want);
    return TVR_OK;
}

// ---- marching cubes (tvr_mesh.hip) --------------------------------------------------------------------------------------------------------------------------
// dims -> points, or a negative status with the message set
static int mesh_points(const char *fn, const int32_t dims[3], long long *points)
{
    if (!dims) return fail(TVR_ERR_INVALID, "%s: dims is NULL", fn);
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 2) return fail(TVR_ERR_INVALID, "%s: dims[%d] = %d, a volume needs at least 2 points along every axis", fn, a, dims[a]);
    const long long n = (long long)dims[0] * dims[1] * dims[2];
    if (3 * n >= (1ll << 31))
        return fail(TVR_ERR_UNSUPPORTED, "%s: %lld points: vertex indices are int32 and 3 * points must stay below 2^31", fn, n);
    *points = n;
    return TVR_OK;
}

size_t tvr_mesh_scratch_bytes(const int32_t dims[3])
{
    long long n;
    if (mesh_points(__func__, dims, &n) != TVR_OK) return 0;
    return mesh_scratch_bytes(n);
}

// a MeshScratch over n elements (marching cubes' and the component filter's)
static int mesh_scratch_check(const char *fn, const void *scratch, size_t scratch_bytes, long long n)
{
    return buffer_check(fn, "scratch", scratch, scratch_bytes, mesh_scratch_bytes(n), "tvr_mesh_scratch_bytes", TVR_ERR_INVALID);
}

int tvr_mesh_count(const float *volume, const int32_t dims[3], float level, void *scratch, size_t scratch_bytes, int64_t *counts_dev, void *stream)
{
    long long n;
    int rc = mesh_points(__func__, dims, &n);
    if (rc != TVR_OK) return rc;
    if (!volume || !counts_dev) return fail(TVR_ERR_INVALID, "%s: volume / counts_dev is NULL", __func__);
    if ((rc = mesh_scratch_check(__func__, scratch, scratch_bytes, n)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_count(volume, dims, level, mesh_carve(n, scratch), (long long *)counts_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_emit(const float *volume, const int32_t dims[3], float level, const float origin[3], const float spacing[3], const void *scratch, size_t scratch_bytes,
                  float *verts, size_t verts_bytes, int64_t n_vertices, int32_t *faces, size_t faces_bytes, int64_t n_triangles, int32_t flip,
                  uint32_t *fault_flag_dev, void *stream)
{
    long long n;
    int rc = mesh_points(__func__, dims, &n);
    if (rc != TVR_OK) return rc;
    if (!volume || !origin || !spacing || !fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: volume / origin / spacing / fault_flag_dev is NULL", __func__);
    if ((rc = mesh_scratch_check(__func__, scratch, scratch_bytes, n)) != TVR_OK) return rc;
    if (n_vertices < 0 || n_vertices > 3 * n || n_triangles < 0 || n_triangles > 5 * n)
        return fail(TVR_ERR_INVALID, "%s: n_vertices %lld / n_triangles %lld outside 0 .. 3 / 5 x %lld points", __func__, (long long)n_vertices, (long long)n_triangles, n);
    if ((n_vertices && !verts) || (n_triangles && !faces)) return fail(TVR_ERR_INVALID, "%s: verts / faces is NULL", __func__);
    if ((rc = out_check(__func__, "verts", verts_bytes, n_vertices, 0, 12, "vertices x 3 fp32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "faces", faces_bytes, n_triangles, 0, 12, "triangles x 3 int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_emit(volume, dims, level, origin, spacing, mesh_carve(n, const_cast<void *>(scratch)), verts, n_vertices, faces, n_triangles, flip, fault_flag_dev,
                             (hipStream_t)stream));
    return TVR_OK;
}

// ---- connected components of a mesh and the component filter (tvr_mesh_cc.hip) ---------------------------------------------------------------------------------
static int cc_counts(const char *fn, int64_t n_vertices, int64_t n_triangles)
{
    return pair_counts(fn, n_vertices, "n_triangles", n_triangles, INT32_MAX, "indices are int32 and both counts must stay below 2^31");
}

size_t tvr_mesh_components_scratch_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (cc_counts(__func__, n_vertices, n_triangles) != TVR_OK) return 0;
    return MESH_CC_SCRATCH_BYTES;
}

int tvr_mesh_components(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, int32_t *vertex_label, size_t vertex_label_bytes, int32_t *component_faces,
                        size_t component_faces_bytes, int64_t *n_components_dev, void *scratch, size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream)
{
    int rc = cc_counts(__func__, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!n_components_dev || !fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: n_components_dev / fault_flag_dev is NULL", __func__);
    if ((n_triangles && !faces) || (n_vertices && (!vertex_label || !component_faces)))
        return fail(TVR_ERR_INVALID, "%s: faces / vertex_label / component_faces is NULL", __func__);
    if (vertex_label_bytes < (size_t)n_vertices * sizeof(int32_t) || component_faces_bytes < (size_t)n_vertices * sizeof(int32_t))
        return fail(TVR_ERR_INVALID, "%s: vertex_label holds %zu B and component_faces %zu B, %lld vertices x int32 need %zu B each", __func__, vertex_label_bytes,
                    component_faces_bytes, (long long)n_vertices, (size_t)n_vertices * 4);
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, MESH_CC_SCRATCH_BYTES, "tvr_mesh_components_scratch_bytes", TVR_ERR_INVALID);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_components(faces, n_triangles, n_vertices, vertex_label, component_faces, (long long *)n_components_dev, scratch, fault_flag_dev,
                                   (hipStream_t)stream));
    return TVR_OK;
}

static long long cc_elements(int64_t n_vertices, int64_t n_triangles) { return n_vertices > n_triangles ? n_vertices : n_triangles; }

size_t tvr_mesh_filter_scratch_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (cc_counts(__func__, n_vertices, n_triangles) != TVR_OK) return 0;
    return mesh_scratch_bytes(cc_elements(n_vertices, n_triangles));
}

int tvr_mesh_filter_count(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const int32_t *vertex_label, const uint8_t *keep_root, void *scratch,
                          size_t scratch_bytes, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = cc_counts(__func__, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!counts_dev || !fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: counts_dev / fault_flag_dev is NULL", __func__);
    if ((n_triangles && !faces) || (n_vertices && (!vertex_label || !keep_root))) return fail(TVR_ERR_INVALID, "%s: faces / vertex_label / keep_root is NULL", __func__);
    const long long n = cc_elements(n_vertices, n_triangles);
    if ((rc = mesh_scratch_check(__func__, scratch, scratch_bytes, n)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_filter_count(faces, n_triangles, n_vertices, vertex_label, keep_root, mesh_carve(n, scratch), (long long *)counts_dev, fault_flag_dev,
                                     (hipStream_t)stream));
    return TVR_OK;
}

// what the two emit passes that shrink a mesh check alike: the output counts against the input's
static int counts_out_check(const char *fn, int64_t n_vertices_out, int64_t n_vertices, int64_t n_triangles_out, int64_t n_triangles)
{
    if (n_vertices_out < 0 || n_vertices_out > n_vertices || n_triangles_out < 0 || n_triangles_out > n_triangles)
        return fail(TVR_ERR_INVALID, "%s: n_vertices_out %lld / n_triangles_out %lld outside 0 .. %lld vertices / %lld triangles", fn, (long long)n_vertices_out,
                    (long long)n_triangles_out, (long long)n_vertices, (long long)n_triangles);
    return TVR_OK;
}

int tvr_mesh_filter_emit(const float *verts, const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const void *scratch, size_t scratch_bytes, float *verts_out,
                         size_t verts_out_bytes, int64_t n_vertices_out, int32_t *faces_out, size_t faces_out_bytes, int64_t n_triangles_out, int32_t *kept_vertex,
                         size_t kept_vertex_bytes, uint32_t *fault_flag_dev, void *stream)
{
    int rc = cc_counts(__func__, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_triangles && !faces) return fail(TVR_ERR_INVALID, "%s: faces is NULL", __func__);
    const long long n = cc_elements(n_vertices, n_triangles);
    if ((rc = mesh_scratch_check(__func__, scratch, scratch_bytes, n)) != TVR_OK) return rc;
    if ((rc = counts_out_check(__func__, n_vertices_out, n_vertices, n_triangles_out, n_triangles)) != TVR_OK) return rc;
    if ((n_vertices_out && (!kept_vertex || (verts && !verts_out))) || (n_triangles_out && !faces_out))
        return fail(TVR_ERR_INVALID, "%s: verts_out / faces_out / kept_vertex is NULL", __func__);
    if (verts && (rc = out_check(__func__, "verts_out", verts_out_bytes, n_vertices_out, 0, 12, "vertices x 3 fp32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "faces_out", faces_out_bytes, n_triangles_out, 0, 12, "triangles x 3 int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "kept_vertex", kept_vertex_bytes, n_vertices_out, 0, 4, "vertices x int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_filter_emit(verts, faces, n_triangles, n_vertices, mesh_carve(n, const_cast<void *>(scratch)), verts_out, n_vertices_out, faces_out, n_triangles_out,
                                    kept_vertex, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- vertex-clustering simplification of a mesh (tvr_mesh_simplify.hip) ----------------------------------------------------------------------------------------
size_t tvr_mesh_simplify_scratch_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (cc_counts(__func__, n_vertices, n_triangles) != TVR_OK) return 0;
    return simplify_carve(n_vertices, n_triangles, nullptr).total;
}

// everything tvr_mesh_simplify_count and _emit share: counts, inputs, lattice, scratch
static int simplify_inputs(const char *fn, const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const float origin[3], const float cell[3],
                           const float inv_cell[3], const void *scratch, size_t scratch_bytes, const uint32_t *fault_flag_dev, SimplifyLattice *lat)
{
    int rc = cc_counts(fn, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!origin || !cell || !inv_cell || !fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: origin / cell / inv_cell / fault_flag_dev is NULL", fn);
    if ((n_vertices && !verts) || (n_triangles && !faces)) return fail(TVR_ERR_INVALID, "%s: verts / faces is NULL", fn);
    for (int a = 0; a < 3; ++a) {
        if (!(cell[a] > 0.0f) || !std::isfinite(cell[a]) || !(inv_cell[a] > 0.0f) || !std::isfinite(inv_cell[a]))
            return fail(TVR_ERR_INVALID, "%s: cell[%d] = %g / inv_cell[%d] = %g: both must be positive and finite", fn, a, (double)cell[a], a, (double)inv_cell[a]);
        lat->origin[a] = origin[a];
        lat->cell[a] = cell[a];
        lat->inv_cell[a] = inv_cell[a];
    }
    return buffer_check(fn, "scratch", scratch, scratch_bytes, simplify_carve(n_vertices, n_triangles, nullptr).total, "tvr_mesh_simplify_scratch_bytes", TVR_ERR_INVALID);
}

int tvr_mesh_simplify_count(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const float origin[3], const float cell[3],
                            const float inv_cell[3], void *scratch, size_t scratch_bytes, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    SimplifyLattice lat;
    const int rc = simplify_inputs(__func__, verts, n_vertices, faces, n_triangles, origin, cell, inv_cell, scratch, scratch_bytes, fault_flag_dev, &lat);
    if (rc != TVR_OK) return rc;
    if (!counts_dev) return fail(TVR_ERR_INVALID, "%s: counts_dev is NULL", __func__);
    HIP_TRY(launch_mesh_simplify_count(verts, n_vertices, faces, n_triangles, lat, simplify_carve(n_vertices, n_triangles, scratch), (long long *)counts_dev,
                                       fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_simplify_emit(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const float origin[3], const float cell[3],
                           const float inv_cell[3], void *scratch, size_t scratch_bytes, float *verts_out, size_t verts_out_bytes, int64_t n_vertices_out,
                           int32_t *faces_out, size_t faces_out_bytes, int64_t n_triangles_out, int32_t *vertex_map, size_t vertex_map_bytes, uint32_t *fault_flag_dev,
                           void *stream)
{
    SimplifyLattice lat;
    int rc = simplify_inputs(__func__, verts, n_vertices, faces, n_triangles, origin, cell, inv_cell, scratch, scratch_bytes, fault_flag_dev, &lat);
    if (rc != TVR_OK) return rc;
    if ((rc = counts_out_check(__func__, n_vertices_out, n_vertices, n_triangles_out, n_triangles)) != TVR_OK) return rc;
    if ((n_vertices_out && !verts_out) || (n_triangles_out && !faces_out) || (n_vertices && !vertex_map))
        return fail(TVR_ERR_INVALID, "%s: verts_out / faces_out / vertex_map is NULL", __func__);
    if ((rc = out_check(__func__, "verts_out", verts_out_bytes, n_vertices_out, 0, 12, "vertices x 3 fp32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "faces_out", faces_out_bytes, n_triangles_out, 0, 12, "triangles x 3 int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "vertex_map", vertex_map_bytes, n_vertices, 0, 4, "vertices x int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_simplify_emit(verts, n_vertices, faces, n_triangles, lat, simplify_carve(n_vertices, n_triangles, scratch), verts_out, n_vertices_out, faces_out,
                                      n_triangles_out, vertex_map, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- vertex adjacency and Taubin smoothing of a mesh (tvr_mesh_smooth.hip) -------------------------------------------------------------------------------------------
static int adj_counts(const char *fn, int64_t n_vertices, int64_t n_triangles)
{
    return pair_counts(fn, n_vertices, "n_triangles", n_triangles, INT32_MAX / 6, "indices are int32, n_vertices and 6 x n_triangles must stay below 2^31");
}

size_t tvr_mesh_adjacency_scratch_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (adj_counts(__func__, n_vertices, n_triangles) != TVR_OK) return 0;
    return adj_carve(n_vertices, n_triangles, nullptr).total;
}

// everything tvr_mesh_adjacency_count and _emit share
static int adj_inputs(const char *fn, const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const void *scratch, size_t scratch_bytes,
                      const uint32_t *fault_flag_dev)
{
    int rc = adj_counts(fn, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", fn);
    if (n_triangles && !faces) return fail(TVR_ERR_INVALID, "%s: faces is NULL", fn);
    return buffer_check(fn, "scratch", scratch, scratch_bytes, adj_carve(n_vertices, n_triangles, nullptr).total, "tvr_mesh_adjacency_scratch_bytes", TVR_ERR_INVALID);
}

int tvr_mesh_adjacency_count(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, void *scratch, size_t scratch_bytes, int64_t *counts_dev,
                             uint32_t *fault_flag_dev, void *stream)
{
    const int rc = adj_inputs(__func__, faces, n_triangles, n_vertices, scratch, scratch_bytes, fault_flag_dev);
    if (rc != TVR_OK) return rc;
    if (!counts_dev) return fail(TVR_ERR_INVALID, "%s: counts_dev is NULL", __func__);
    HIP_TRY(launch_mesh_adjacency_count(faces, n_triangles, n_vertices, adj_carve(n_vertices, n_triangles, scratch), (long long *)counts_dev, fault_flag_dev,
                                        (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_adjacency_emit(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, const void *scratch, size_t scratch_bytes, int32_t *offsets,
                            size_t offsets_bytes, int32_t *neighbours, size_t neighbours_bytes, int32_t *edge_faces, size_t edge_faces_bytes, int64_t n_half_edges,
                            uint32_t *fault_flag_dev, void *stream)
{
    int rc = adj_inputs(__func__, faces, n_triangles, n_vertices, scratch, scratch_bytes, fault_flag_dev);
    if (rc != TVR_OK) return rc;
    if (n_half_edges < 0 || n_half_edges > 6 * n_triangles)
        return fail(TVR_ERR_INVALID, "%s: n_half_edges %lld outside 0 .. 6 x %lld triangles", __func__, (long long)n_half_edges, (long long)n_triangles);
    if (!offsets || (n_half_edges && (!neighbours || !edge_faces))) return fail(TVR_ERR_INVALID, "%s: offsets / neighbours / edge_faces is NULL", __func__);
    if ((rc = out_check(__func__, "offsets", offsets_bytes, n_vertices, 1, 4, "vertices + 1 x int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "neighbours", neighbours_bytes, n_half_edges, 0, 4, "half-edges x int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    if ((rc = out_check(__func__, "edge_faces", edge_faces_bytes, n_half_edges, 0, 4, "half-edges x int32", TVR_ERR_INVALID)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_adjacency_emit(n_vertices, adj_carve(n_vertices, n_triangles, const_cast<void *>(scratch)), offsets, neighbours, edge_faces, n_half_edges,
                                       fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

static int smooth_counts(const char *fn, int64_t n_vertices, int64_t n_half_edges)
{
    return pair_counts(fn, n_vertices, "n_half_edges", n_half_edges, INT32_MAX, "indices are int32 and both counts must stay below 2^31");
}

size_t tvr_mesh_smooth_scratch_bytes(int64_t n_vertices, int64_t n_half_edges)
{
    if (smooth_counts(__func__, n_vertices, n_half_edges) != TVR_OK) return 0;
    return smooth_carve(n_vertices, nullptr).total;
}

int tvr_mesh_smooth(const float *verts, int64_t n_vertices, const int32_t *offsets, const int32_t *neighbours, const int32_t *edge_faces, int64_t n_half_edges,
                    int32_t iterations, float lambda, float mu, int32_t pin_boundary, void *scratch, size_t scratch_bytes, float *verts_out, size_t verts_out_bytes,
                    uint32_t *fault_flag_dev, void *stream)
{
    int rc = smooth_counts(__func__, n_vertices, n_half_edges);
    if (rc != TVR_OK) return rc;
    if (iterations < 0 || iterations > TVR_MESH_SMOOTH_MAX_ITERATIONS)
        return fail(TVR_ERR_INVALID, "%s: iterations %d outside 0 .. %d", __func__, (int)iterations, TVR_MESH_SMOOTH_MAX_ITERATIONS);
    if (!std::isfinite(lambda) || !std::isfinite(mu)) return fail(TVR_ERR_INVALID, "%s: lambda = %g / mu = %g: both must be finite", __func__, (double)lambda, (double)mu);
    if (!fault_flag_dev || !offsets) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev / offsets is NULL", __func__);
    if ((n_vertices && (!verts || !verts_out)) || (n_half_edges && !neighbours)) return fail(TVR_ERR_INVALID, "%s: verts / verts_out / neighbours is NULL", __func__);
    if (pin_boundary && n_half_edges && !edge_faces) return fail(TVR_ERR_INVALID, "%s: edge_faces is NULL and pin_boundary is set", __func__);
    if (verts_out_bytes != (size_t)n_vertices * 3 * sizeof(float))
        return fail(TVR_ERR_INVALID, "%s: verts_out holds %zu B, %lld vertices x 3 fp32 are %zu B", __func__, verts_out_bytes, (long long)n_vertices,
                    (size_t)n_vertices * 12);
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, smooth_carve(n_vertices, nullptr).total, "tvr_mesh_smooth_scratch_bytes", TVR_ERR_INVALID);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_smooth(verts, n_vertices, offsets, neighbours, pin_boundary && n_half_edges ? edge_faces : nullptr, n_half_edges, iterations, lambda, mu,
                               smooth_carve(n_vertices, scratch), verts_out, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- z-buffer rasteriser of indexed triangle meshes (tvr_mesh_raster.hip) -------------------------------------------------------------------------------------------------
static int raster_counts(const char *fn, int64_t n_triangles, int64_t H, int64_t W)
{
    if (n_triangles < 0) return fail(TVR_ERR_INVALID, "%s: n_triangles = %lld is negative", fn, (long long)n_triangles);
    if (H < 1 || W < 1) return fail(TVR_ERR_INVALID, "%s: H = %lld, W = %lld: an image has at least one row and one column", fn, (long long)H, (long long)W);
    if (H > TVR_MESH_RASTER_MAX_SIDE || W > TVR_MESH_RASTER_MAX_SIDE)
        return fail(TVR_ERR_UNSUPPORTED, "%s: H = %lld, W = %lld: a side above 2^24 = %d pixels is not taken (pixel centres i + .5 and the box's float clamp are exact "
                    "only up to there)", fn, (long long)H, (long long)W, TVR_MESH_RASTER_MAX_SIDE);
    if (H * W > INT32_MAX || n_triangles > INT32_MAX)
        return fail(TVR_ERR_UNSUPPORTED, "%s: H * W = %lld / n_triangles = %lld: pixel and triangle indices are int32 and both counts must stay below 2^31", fn,
                    (long long)(H * W), (long long)n_triangles);
    return TVR_OK;
}

size_t tvr_mesh_raster_scratch_bytes(int64_t n_triangles, int32_t H, int32_t W)
{
    if (raster_counts(__func__, n_triangles, H, W) != TVR_OK) return 0;
    return mesh_raster_scratch_bytes(n_triangles, (long long)H * W);
}

int tvr_mesh_raster(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const tvr_mesh_camera *cam, const float *attr, int32_t n_attr,
                    float *depth, size_t depth_bytes, int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes, float *attr_out, size_t attr_out_bytes, void *scratch,
                    size_t scratch_bytes, int32_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    if (!cam) return fail(TVR_ERR_INVALID, "%s: cam is NULL", __func__);
    if (!depth || !tri || !bary || !scratch || !counts_dev || !fault_flag_dev)
        return fail(TVR_ERR_INVALID, "%s: depth / tri / bary / scratch / counts_dev / fault_flag_dev is NULL", __func__);
    int rc = count_check(__func__, "n_vertices", n_vertices, INT64_MAX, "");
    if (rc != TVR_OK) return rc;
    if (n_triangles > 0 && (!faces || !verts)) return fail(TVR_ERR_INVALID, "%s: faces / verts is NULL with %lld triangles", __func__, (long long)n_triangles);
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(cam->c2w[k])) return fail(TVR_ERR_INVALID, "%s: cam->c2w[%d] = %g is not finite", __func__, k, (double)cam->c2w[k]);
    if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !(cam->fx > 0.0f) || !(cam->fy > 0.0f))
        return fail(TVR_ERR_INVALID, "%s: fx = %g, fy = %g must be finite and > 0", __func__, (double)cam->fx, (double)cam->fy);
    if (!std::isfinite(cam->cx) || !std::isfinite(cam->cy)) return fail(TVR_ERR_INVALID, "%s: cx = %g, cy = %g must be finite", __func__, (double)cam->cx, (double)cam->cy);
    if (!std::isfinite(cam->near_) || cam->near_ < 0.0f) return fail(TVR_ERR_INVALID, "%s: near = %g must be finite and >= 0", __func__, (double)cam->near_);
    if (cam->cull != 0 && cam->cull != 1) return fail(TVR_ERR_INVALID, "%s: cull = %d is neither 0 nor 1", __func__, (int)cam->cull);
    if (cam->large_bbox < 0) return fail(TVR_ERR_INVALID, "%s: large_bbox = %d is negative (0 = the default of %d pixels)", __func__, (int)cam->large_bbox,
                                         TVR_MESH_RASTER_LARGE_BBOX);
    if (n_attr < 0 || n_attr > TVR_MESH_RASTER_MAX_ATTR) return fail(TVR_ERR_INVALID, "%s: n_attr = %d outside 0 .. %d", __func__, (int)n_attr, TVR_MESH_RASTER_MAX_ATTR);
    if (n_attr > 0 && (!attr || !attr_out)) return fail(TVR_ERR_INVALID, "%s: attr / attr_out is NULL with n_attr = %d", __func__, (int)n_attr);
    if ((rc = raster_counts(__func__, n_triangles, cam->H, cam->W)) != TVR_OK) return rc;
    if ((rc = count_check(__func__, "n_vertices", n_vertices, INT32_MAX, "vertex indices are int32")) != TVR_OK) return rc;
    // the scratch is known not to be NULL; its alignment is reported before the outputs' sizes and its own size after them
    if ((rc = buffer_check(__func__, "scratch", scratch, 0, 0, "", TVR_ERR_SCRATCH)) != TVR_OK) return rc;
    const int64_t n_pixels = (int64_t)cam->H * cam->W;
    NEED("depth [H*W]", depth_bytes, n_pixels, 1);
    NEED("tri [H*W]", tri_bytes, n_pixels, 1);
    NEED("bary [H*W,3]", bary_bytes, n_pixels, 3);
    if (n_attr > 0) NEED("attr_out [H*W,n_attr]", attr_out_bytes, n_pixels, n_attr);
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, mesh_raster_scratch_bytes(n_triangles, n_pixels), "tvr_mesh_raster_scratch_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_raster(verts, n_vertices, faces, n_triangles, *cam, n_attr > 0 ? attr : nullptr, n_attr, depth, tri, bary, n_attr > 0 ? attr_out : nullptr, scratch,
                               (int *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- per-triangle texture atlas (tvr_mesh_texture.hip) ---------------------------------------------------------------------------------------------------------------------
// the atlas of F triangles at patch side P with C squares per row: *Ha, *Wa; every count in range and fewer than 2^31 texels, else an error that names the argument
static int atlas_layout(const char *fn, int64_t n_triangles, int32_t P, int32_t C, int64_t *Ha, int64_t *Wa)
{
    if (n_triangles < 0) return fail(TVR_ERR_INVALID, "%s: n_triangles = %lld is negative", fn, (long long)n_triangles);
    if (P < TVR_MESH_ATLAS_MIN_P || P > TVR_MESH_ATLAS_MAX_P)
        return fail(TVR_ERR_INVALID, "%s: P = %d outside %d .. %d texels per patch side", fn, (int)P, TVR_MESH_ATLAS_MIN_P, TVR_MESH_ATLAS_MAX_P);
    if (C < 1) return fail(TVR_ERR_INVALID, "%s: C = %d: an atlas row holds at least one square", fn, (int)C);
    if (n_triangles > INT32_MAX) return fail(TVR_ERR_UNSUPPORTED, "%s: n_triangles = %lld: triangle indices are int32", fn, (long long)n_triangles);
    const int64_t S = (n_triangles + 1) / 2, rows = S > 0 ? (S + C - 1) / C : 1;
    *Wa = (int64_t)C * P;
    *Ha = rows * P;
    if (*Wa > INT32_MAX || *Ha > INT32_MAX || *Ha * *Wa > INT32_MAX)
        return fail(TVR_ERR_UNSUPPORTED, "%s: an atlas of Ha = %lld x Wa = %lld texels (n_triangles = %lld, P = %d, C = %d): texel indices are int32 and Ha * Wa must stay "
                    "below 2^31", fn, (long long)*Ha, (long long)*Wa, (long long)n_triangles, (int)P, (int)C);
    return TVR_OK;
}

int tvr_mesh_atlas_points(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t P, int32_t C, int64_t texel0, int64_t n,
                          float *pos_out, size_t pos_bytes, int32_t *tri_out, size_t tri_bytes, uint32_t *fault_flag_dev, void *stream)
{
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    int rc = count_check(__func__, "n_vertices", n_vertices, INT64_MAX, "");
    if (rc != TVR_OK) return rc;
    int64_t Ha, Wa;
    if ((rc = atlas_layout(__func__, n_triangles, P, C, &Ha, &Wa)) != TVR_OK) return rc;
    if ((rc = count_check(__func__, "n_vertices", n_vertices, INT32_MAX, "vertex indices are int32")) != TVR_OK) return rc;
    if (n_triangles > 0 && (!faces || !verts)) return fail(TVR_ERR_INVALID, "%s: faces / verts is NULL with %lld triangles", __func__, (long long)n_triangles);
    if (texel0 < 0 || n < 0 || texel0 > Ha * Wa || n > Ha * Wa - texel0)
        return fail(TVR_ERR_INVALID, "%s: texel0 = %lld, n = %lld: the range leaves the atlas of %lld x %lld = %lld texels", __func__, (long long)texel0, (long long)n,
                    (long long)Ha, (long long)Wa, (long long)(Ha * Wa));
    if (n > 0 && (!pos_out || !tri_out)) return fail(TVR_ERR_INVALID, "%s: pos_out / tri_out is NULL with n = %lld texels", __func__, (long long)n);
    NEED("pos_out [n,3]", pos_bytes, n, 3);
    NEED("tri_out [n]", tri_bytes, n, 1);
    HIP_TRY(launch_mesh_atlas_points(verts, n_vertices, faces, n_triangles, P, C, texel0, n, pos_out, tri_out, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_texture_sample(const int32_t *tri, const float *bary, int64_t n_pix, const void *atlas, int32_t fmt, int32_t Ha, int32_t Wa, int32_t P, int32_t C,
                            int64_t n_triangles, float *out, size_t out_bytes, void *stream)
{
    int rc = count_check(__func__, "n_pix", n_pix, INT64_MAX, "");
    if (rc != TVR_OK) return rc;
    if (fmt != 0 && fmt != 1) return fail(TVR_ERR_INVALID, "%s: fmt = %d is neither 0 (uint8 RGB) nor 1 (fp32 RGB)", __func__, (int)fmt);
    int64_t ha, wa;
    if ((rc = atlas_layout(__func__, n_triangles, P, C, &ha, &wa)) != TVR_OK) return rc;
    if (Ha != ha || Wa != wa)
        return fail(TVR_ERR_INVALID, "%s: Ha = %d, Wa = %d, but %lld triangles at P = %d, C = %d make an atlas of %lld x %lld", __func__, (int)Ha, (int)Wa,
                    (long long)n_triangles, (int)P, (int)C, (long long)ha, (long long)wa);
    if ((rc = count_check(__func__, "n_pix", n_pix, INT32_MAX, "pixel indices are int32")) != TVR_OK) return rc;
    if (!atlas) return fail(TVR_ERR_INVALID, "%s: atlas is NULL", __func__);
    if (n_pix > 0 && (!tri || !bary || !out)) return fail(TVR_ERR_INVALID, "%s: tri / bary / out is NULL with n_pix = %lld", __func__, (long long)n_pix);
    NEED("out [n_pix,3]", out_bytes, n_pix, 3);
    HIP_TRY(launch_mesh_texture_sample(tri, bary, n_pix, atlas, fmt, ha * wa, P, C, n_triangles, out, (hipStream_t)stream));
    return TVR_OK;
}

// ---- linear BVH over a mesh's triangles, ray casts and ambient occlusion (tvr_mesh_bvh.hip) ----------------------------------------------------------------------------
static int bvh_counts(const char *fn, int64_t n_triangles)
{
    if (n_triangles < 0) return fail(TVR_ERR_INVALID, "%s: n_triangles = %lld is negative", fn, (long long)n_triangles);
    if (n_triangles > TVR_MESH_BVH_MAX_TRIANGLES)
        return fail(TVR_ERR_UNSUPPORTED, "%s: n_triangles = %lld: at most TVR_MESH_BVH_MAX_TRIANGLES = %d (the 2F - 1 node indices are int32)", fn, (long long)n_triangles,
                    TVR_MESH_BVH_MAX_TRIANGLES);
    return TVR_OK;
}

// the counts of a mesh under a hierarchy (all the pseudo-normal table's queries check)
static int bvh_mesh_counts(const char *fn, int64_t n_vertices, int64_t n_triangles)
{
    const int rc = bvh_counts(fn, n_triangles);
    if (rc != TVR_OK) return rc;
    return count_check(fn, "n_vertices", n_vertices, INT32_MAX, "vertex indices are int32");
}

// what every call that reads a mesh checks: counts, pointers
static int bvh_mesh(const char *fn, const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles)
{
    const int rc = bvh_mesh_counts(fn, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (n_triangles > 0 && (!faces || !verts)) return fail(TVR_ERR_INVALID, "%s: faces / verts is NULL with %lld triangles", fn, (long long)n_triangles);
    return TVR_OK;
}

// the hierarchy's blob, as every query takes it
static int bvh_blob(const char *fn, const void *bvh, size_t bvh_bytes, int64_t n_triangles)
{
    return buffer_check(fn, "bvh", bvh, bvh_bytes, mesh_bvh_bytes(n_triangles, nullptr), "tvr_mesh_bvh_bytes", TVR_ERR_SCRATCH);
}

// the query points of tvr_mesh_bvh_signed and tvr_mesh_winding_query: an array of n_points, or the lattice, whose point count then replaces *n_points
static int lattice_points(const char *fn, const float *points, const tvr_mesh_lattice *lattice, int64_t *n_points)
{
    if (points && lattice) return fail(TVR_ERR_INVALID, "%s: both points and lattice are given", fn);
    if (lattice) {
        for (int k = 0; k < 3; ++k) {
            if (lattice->dims[k] < 0) return fail(TVR_ERR_INVALID, "%s: lattice dims[%d] = %d is negative", fn, k, (int)lattice->dims[k]);
            if (!std::isfinite(lattice->origin[k]) || !std::isfinite(lattice->spacing[k]))
                return fail(TVR_ERR_INVALID, "%s: lattice origin[%d] = %g / spacing[%d] = %g is not finite", fn, k, (double)lattice->origin[k], k,
                            (double)lattice->spacing[k]);
        }
        const double total = (double)lattice->dims[0] * (double)lattice->dims[1] * (double)lattice->dims[2];
        if (total > (double)INT32_MAX) return fail(TVR_ERR_UNSUPPORTED, "%s: the lattice holds %.0f points: at most 2^31 - 1 per call", fn, total);
        *n_points = (int64_t)lattice->dims[0] * lattice->dims[1] * lattice->dims[2];
    }
    return count_check(fn, "n_points", *n_points, INT32_MAX, "at most 2^31 - 1 points per call");
}

// a table built beside the hierarchy (pseudo-normals, winding moments) as a query takes it: a buffer of exactly the size the mesh's counts give.  n_vertices < 0:
// the table's size depends on the triangles alone
static int table_check(const char *fn, const void *table, size_t table_bytes, size_t want, const char *query, int64_t n_vertices, int64_t n_triangles)
{
    const int rc = buffer_check(fn, "table", table, table_bytes, want, query, TVR_ERR_SCRATCH);
    if (rc != TVR_OK || table_bytes == want) return rc;
    char verts[40] = "";
    if (n_vertices >= 0) snprintf(verts, sizeof(verts), "%lld vertices and ", (long long)n_vertices);
    return fail(TVR_ERR_SCRATCH, "%s: table holds %zu B, the table of %s%lld triangles is %zu B: it belongs to another mesh", fn, table_bytes, verts, (long long)n_triangles,
                want);
}

size_t tvr_mesh_bvh_bytes(int64_t n_triangles)
{
    if (bvh_counts(__func__, n_triangles) != TVR_OK) return 0;
    return mesh_bvh_bytes(n_triangles, nullptr);
}

size_t tvr_mesh_bvh_scratch_bytes(int64_t n_triangles)
{
    if (bvh_counts(__func__, n_triangles) != TVR_OK) return 0;
    return mesh_bvh_scratch_bytes(n_triangles);
}

int tvr_mesh_bvh_describe(int64_t n_triangles, tvr_mesh_bvh_layout *out)
{
    if (!out) return fail(TVR_ERR_INVALID, "%s: out is NULL", __func__);
    const int rc = bvh_counts(__func__, n_triangles);
    if (rc != TVR_OK) return rc;
    MeshBvhCarve c;
    mesh_bvh_bytes(n_triangles, &c);
    out->header = c.header; out->boxes = c.box; out->children = c.child; out->leaf_order = c.leaf_tri; out->total = c.total;
    out->box_stride = 6 * sizeof(float); out->child_stride = 2 * sizeof(int32_t); out->leaf_stride = sizeof(int32_t);
    out->n_nodes = n_triangles ? 2 * (size_t)n_triangles - 1 : 0;
    out->n_internal = n_triangles ? (size_t)n_triangles - 1 : 0;
    return TVR_OK;
}

int tvr_mesh_bvh_keys(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, uint64_t *keys_out, size_t keys_bytes, void *scratch,
                      size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_triangles > 0 && !keys_out) return fail(TVR_ERR_INVALID, "%s: keys_out is NULL with %lld triangles", __func__, (long long)n_triangles);
    if (keys_out && (uintptr_t)keys_out % 8) return fail(TVR_ERR_INVALID, "%s: keys_out is not 8-byte aligned", __func__);
    if ((rc = out_check(__func__, "keys_out", keys_bytes, n_triangles, 0, 8, "triangles x uint64", TVR_ERR_SCRATCH)) != TVR_OK) return rc;
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, mesh_bvh_scratch_bytes(n_triangles), "tvr_mesh_bvh_scratch_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_bvh_keys(verts, n_vertices, faces, n_triangles, (unsigned long long *)keys_out, scratch, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_bvh_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const uint64_t *sorted_keys, void *bvh, size_t bvh_bytes,
                       void *scratch, size_t scratch_bytes, int32_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_triangles > 0 && !sorted_keys) return fail(TVR_ERR_INVALID, "%s: sorted_keys is NULL with %lld triangles", __func__, (long long)n_triangles);
    if (sorted_keys && (uintptr_t)sorted_keys % 8) return fail(TVR_ERR_INVALID, "%s: sorted_keys is not 8-byte aligned", __func__);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, mesh_bvh_scratch_bytes(n_triangles), "tvr_mesh_bvh_scratch_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_bvh_build(verts, n_vertices, faces, n_triangles, (const unsigned long long *)sorted_keys, bvh, scratch, (int *)counts_dev, fault_flag_dev,
                                  (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_bvh_cast(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *origins,
                      const float *dirs, int64_t n_rays, float t_min, float t_max, int32_t mode, int32_t cull, float *t, size_t t_bytes, int32_t *tri, size_t tri_bytes,
                      float *bary, size_t bary_bytes, uint8_t *hit, size_t hit_bytes, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if ((rc = count_check(__func__, "n_rays", n_rays, INT32_MAX, "at most 2^31 - 1 rays per call")) != TVR_OK) return rc;
    if (mode != TVR_MESH_BVH_CLOSEST && mode != TVR_MESH_BVH_ANY) return fail(TVR_ERR_INVALID, "%s: mode = %d is neither 0 (closest hit) nor 1 (any hit)", __func__, (int)mode);
    if (cull != 0 && cull != 1) return fail(TVR_ERR_INVALID, "%s: cull = %d is neither 0 nor 1", __func__, (int)cull);
    if (std::isnan(t_min) || std::isnan(t_max)) return fail(TVR_ERR_INVALID, "%s: t_min = %g / t_max = %g is NaN", __func__, (double)t_min, (double)t_max);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    if (n_rays > 0 && (!origins || !dirs)) return fail(TVR_ERR_INVALID, "%s: origins / dirs is NULL with %lld rays", __func__, (long long)n_rays);
    if (mode == TVR_MESH_BVH_ANY) {
        if (n_rays > 0 && !hit) return fail(TVR_ERR_INVALID, "%s: hit is NULL in any-hit mode", __func__);
        if (hit_bytes < (size_t)n_rays) return fail(TVR_ERR_SCRATCH, "%s: hit holds %zu B, the kernel writes %lld uint8", __func__, hit_bytes, (long long)n_rays);
    } else {
        if (n_rays > 0 && (!t || !tri || !bary)) return fail(TVR_ERR_INVALID, "%s: t / tri / bary is NULL in closest-hit mode", __func__);
        NEED("t [n_rays]", t_bytes, n_rays, 1);
        NEED("tri [n_rays]", tri_bytes, n_rays, 1);
        NEED("bary [n_rays,3]", bary_bytes, n_rays, 3);
    }
    HIP_TRY(launch_mesh_bvh_cast(verts, n_vertices, faces, n_triangles, bvh, origins, dirs, n_rays, t_min, t_max, mode == TVR_MESH_BVH_ANY, cull, t, tri, bary, hit,
                                 (unsigned long long *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_bvh_occlusion(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *points,
                           const float *normals, int64_t n_points, const float *dirs, int32_t n_dirs, float bias, float t_max, float *out, size_t out_bytes,
                           int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_points < 0 || n_dirs < 0) return fail(TVR_ERR_INVALID, "%s: n_points = %lld / n_dirs = %d is negative", __func__, (long long)n_points, (int)n_dirs);
    if ((rc = count_check(__func__, "n_points", n_points, INT32_MAX, "at most 2^31 - 1 points per call")) != TVR_OK) return rc;
    if (n_dirs > TVR_MESH_BVH_MAX_DIRS) return fail(TVR_ERR_INVALID, "%s: n_dirs = %d above TVR_MESH_BVH_MAX_DIRS = %d", __func__, (int)n_dirs, TVR_MESH_BVH_MAX_DIRS);
    if (!std::isfinite(bias)) return fail(TVR_ERR_INVALID, "%s: bias = %g must be finite", __func__, (double)bias);
    if (std::isnan(t_max)) return fail(TVR_ERR_INVALID, "%s: t_max is NaN", __func__);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    if (n_points > 0 && (!points || !normals || !out)) return fail(TVR_ERR_INVALID, "%s: points / normals / out is NULL with %lld points", __func__, (long long)n_points);
    if (n_dirs > 0 && !dirs) return fail(TVR_ERR_INVALID, "%s: dirs is NULL with n_dirs = %d", __func__, (int)n_dirs);
    NEED("out [n_points]", out_bytes, n_points, 1);
    HIP_TRY(launch_mesh_bvh_occlusion(verts, n_vertices, faces, n_triangles, bvh, points, normals, n_points, dirs, n_dirs, bias, t_max, out,
                                      (unsigned long long *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_bvh_nearest(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const float *points,
                         int64_t n_points, float max_dist, float *dist, size_t dist_bytes, int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes,
                         int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if ((rc = count_check(__func__, "n_points", n_points, INT32_MAX, "at most 2^31 - 1 points per call")) != TVR_OK) return rc;
    if (std::isnan(max_dist) || max_dist < 0.0f) return fail(TVR_ERR_INVALID, "%s: max_dist = %g is NaN or negative", __func__, (double)max_dist);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    if (n_points > 0 && (!points || !dist || !tri || !bary)) return fail(TVR_ERR_INVALID, "%s: points / dist / tri / bary is NULL with %lld points", __func__, (long long)n_points);
    NEED("dist [n_points]", dist_bytes, n_points, 1);
    NEED("tri [n_points]", tri_bytes, n_points, 1);
    NEED("bary [n_points,3]", bary_bytes, n_points, 3);
    HIP_TRY(launch_mesh_bvh_nearest(verts, n_vertices, faces, n_triangles, bvh, points, n_points, max_dist, dist, tri, bary, (unsigned long long *)counts_dev,
                                    fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- pseudo-normal table and the signed closest-point query (tvr_mesh_pseudo.hip, tvr_mesh_bvh.hip bv_signed_kernel) ------------------------------------------------------------
size_t tvr_mesh_pseudonormals_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (bvh_mesh_counts(__func__, n_vertices, n_triangles) != TVR_OK) return 0;
    return mesh_pseudo_bytes(n_vertices, n_triangles, nullptr);
}

size_t tvr_mesh_pseudonormals_scratch_bytes(int64_t n_triangles)
{
    if (bvh_counts(__func__, n_triangles) != TVR_OK) return 0;
    return mesh_pseudo_scratch_bytes(n_triangles);
}

int tvr_mesh_pseudonormals_describe(int64_t n_vertices, int64_t n_triangles, tvr_mesh_pseudonormals_layout *out)
{
    if (!out) return fail(TVR_ERR_INVALID, "%s: out is NULL", __func__);
    const int rc = bvh_mesh_counts(__func__, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    MeshPseudoCarve c;
    mesh_pseudo_bytes(n_vertices, n_triangles, &c);
    out->header = c.header; out->face_n = c.face_n; out->edge_n = c.edge_n; out->vert_n = c.vert_n; out->total = c.total;
    out->face_stride = 3 * sizeof(float); out->edge_stride = 9 * sizeof(float); out->vert_stride = 3 * sizeof(float);
    return TVR_OK;
}

int tvr_mesh_pseudonormals_keys(const int32_t *faces, int64_t n_vertices, int64_t n_triangles, uint64_t *corner_keys_out, uint64_t *edge_keys_out, size_t keys_bytes,
                                uint32_t *fault_flag_dev, void *stream)
{
    const int rc = bvh_mesh_counts(__func__, n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_triangles > 0 && (!faces || !corner_keys_out || !edge_keys_out))
        return fail(TVR_ERR_INVALID, "%s: faces / corner_keys_out / edge_keys_out is NULL with %lld triangles", __func__, (long long)n_triangles);
    if ((uintptr_t)corner_keys_out % 8 || (uintptr_t)edge_keys_out % 8) return fail(TVR_ERR_INVALID, "%s: corner_keys_out / edge_keys_out is not 8-byte aligned", __func__);
    if (keys_bytes < (size_t)n_triangles * 3 * sizeof(uint64_t))
        return fail(TVR_ERR_SCRATCH, "%s: each key array holds %zu B, 3 x %lld corners x uint64 need %zu B", __func__, keys_bytes, (long long)n_triangles,
                    (size_t)n_triangles * 24);
    HIP_TRY(launch_mesh_pseudo_keys(faces, n_vertices, n_triangles, (unsigned long long *)corner_keys_out, (unsigned long long *)edge_keys_out, fault_flag_dev,
                                    (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_pseudonormals_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const uint64_t *sorted_corner_keys,
                                 const uint64_t *sorted_edge_keys, const int64_t *edge_order, void *table, size_t table_bytes, void *scratch, size_t scratch_bytes,
                                 int32_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (n_triangles > 0 && (!sorted_corner_keys || !sorted_edge_keys || !edge_order))
        return fail(TVR_ERR_INVALID, "%s: sorted_corner_keys / sorted_edge_keys / edge_order is NULL with %lld triangles", __func__, (long long)n_triangles);
    if ((uintptr_t)sorted_corner_keys % 8 || (uintptr_t)sorted_edge_keys % 8 || (uintptr_t)edge_order % 8)
        return fail(TVR_ERR_INVALID, "%s: sorted_corner_keys / sorted_edge_keys / edge_order is not 8-byte aligned", __func__);
    rc = buffer_check(__func__, "table", table, table_bytes, mesh_pseudo_bytes(n_vertices, n_triangles, nullptr), "tvr_mesh_pseudonormals_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, mesh_pseudo_scratch_bytes(n_triangles), "tvr_mesh_pseudonormals_scratch_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_pseudo_build(verts, n_vertices, faces, n_triangles, (const unsigned long long *)sorted_corner_keys, (const unsigned long long *)sorted_edge_keys,
                                     (const long long *)edge_order, table, scratch, (int *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_bvh_signed(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const void *table,
                        size_t table_bytes, const float *points, int64_t n_points, const tvr_mesh_lattice *lattice, float max_dist, float *sdist, size_t sdist_bytes,
                        int32_t *tri, size_t tri_bytes, float *bary, size_t bary_bytes, int8_t *feature, size_t feature_bytes, int64_t *counts_dev,
                        uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if ((rc = lattice_points(__func__, points, lattice, &n_points)) != TVR_OK) return rc;
    if (std::isnan(max_dist) || max_dist < 0.0f) return fail(TVR_ERR_INVALID, "%s: max_dist = %g is NaN or negative", __func__, (double)max_dist);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    rc = table_check(__func__, table, table_bytes, mesh_pseudo_bytes(n_vertices, n_triangles, nullptr), "tvr_mesh_pseudonormals_bytes", n_vertices, n_triangles);
    if (rc != TVR_OK) return rc;
    if (n_points > 0 && ((!points && !lattice) || !sdist)) return fail(TVR_ERR_INVALID, "%s: points (or lattice) / sdist is NULL with %lld points", __func__, (long long)n_points);
    NEED("sdist [n_points]", sdist_bytes, n_points, 1);
    if (tri) NEED("tri [n_points]", tri_bytes, n_points, 1);
    if (bary) NEED("bary [n_points,3]", bary_bytes, n_points, 3);
    if (feature && feature_bytes < (size_t)n_points)
        return fail(TVR_ERR_SCRATCH, "%s: feature holds %zu B, the kernel writes %lld int8", __func__, feature_bytes, (long long)n_points);
    HIP_TRY(launch_mesh_bvh_signed(verts, n_vertices, faces, n_triangles, bvh, table, points, lattice ? lattice->origin : nullptr, lattice ? lattice->spacing : nullptr,
                                   lattice ? lattice->dims : nullptr, n_points, max_dist, sdist, tri, bary, (signed char *)feature, (unsigned long long *)counts_dev,
                                   fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- node moments beside the hierarchy and the winding-number query (tvr_mesh_winding.hip) ------------------------------------------------------------------------------------
size_t tvr_mesh_winding_bytes(int64_t n_triangles)
{
    if (bvh_counts(__func__, n_triangles) != TVR_OK) return 0;
    return mesh_winding_bytes(n_triangles, nullptr);
}

size_t tvr_mesh_winding_scratch_bytes(int64_t n_triangles)
{
    if (bvh_counts(__func__, n_triangles) != TVR_OK) return 0;
    return mesh_winding_scratch_bytes(n_triangles);
}

int tvr_mesh_winding_describe(int64_t n_triangles, tvr_mesh_winding_layout *out)
{
    if (!out) return fail(TVR_ERR_INVALID, "%s: out is NULL", __func__);
    const int rc = bvh_counts(__func__, n_triangles);
    if (rc != TVR_OK) return rc;
    MeshWindingCarve c;
    mesh_winding_bytes(n_triangles, &c);
    out->header = c.header; out->rows = c.rows; out->total = c.total;
    out->row_stride = 8 * sizeof(float);
    out->n_rows = n_triangles ? (size_t)n_triangles - 1 : 0;
    return TVR_OK;
}

int tvr_mesh_winding_build(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, void *table,
                           size_t table_bytes, void *scratch, size_t scratch_bytes, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    rc = buffer_check(__func__, "table", table, table_bytes, mesh_winding_bytes(n_triangles, nullptr), "tvr_mesh_winding_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    rc = buffer_check(__func__, "scratch", scratch, scratch_bytes, mesh_winding_scratch_bytes(n_triangles), "tvr_mesh_winding_scratch_bytes", TVR_ERR_SCRATCH);
    if (rc != TVR_OK) return rc;
    HIP_TRY(launch_mesh_winding_build(verts, n_vertices, faces, n_triangles, bvh, table, scratch, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_winding_query(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, const void *table,
                           size_t table_bytes, const float *points, int64_t n_points, const tvr_mesh_lattice *lattice, float beta, float *w, size_t w_bytes,
                           int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = bvh_mesh(__func__, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", __func__);
    if (!(beta >= 1.0f)) return fail(TVR_ERR_INVALID, "%s: beta = %g must lie in 1 .. +inf (+inf = the exact sum)", __func__, (double)beta);
    if ((rc = lattice_points(__func__, points, lattice, &n_points)) != TVR_OK) return rc;
    if ((rc = bvh_blob(__func__, bvh, bvh_bytes, n_triangles)) != TVR_OK) return rc;
    if ((rc = table_check(__func__, table, table_bytes, mesh_winding_bytes(n_triangles, nullptr), "tvr_mesh_winding_bytes", -1, n_triangles)) != TVR_OK) return rc;
    if (n_points > 0 && ((!points && !lattice) || !w)) return fail(TVR_ERR_INVALID, "%s: points (or lattice) / w is NULL with %lld points", __func__, (long long)n_points);
    NEED("w [n_points]", w_bytes, n_points, 1);
    HIP_TRY(launch_mesh_winding_query(verts, n_vertices, faces, n_triangles, bvh, table, points, lattice ? lattice->origin : nullptr, lattice ? lattice->spacing : nullptr,
                                      lattice ? lattice->dims : nullptr, n_points, beta, w, (unsigned long long *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

// ---- the triangle-pair query on the hierarchy (tvr_mesh_crossings.hip) ----------------------------------------------------------------------------------------------------------
// what both passes check: the hierarchy's mesh and blob, the mode, the query mesh
static int crossings_args(const char *fn, const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, int32_t mode,
                          const float *verts_q, int64_t n_vertices_q, const int32_t *faces_q, int64_t n_triangles_q, const uint32_t *fault_flag_dev)
{
    int rc = bvh_mesh(fn, verts, n_vertices, faces, n_triangles);
    if (rc != TVR_OK) return rc;
    if (!fault_flag_dev) return fail(TVR_ERR_INVALID, "%s: fault_flag_dev is NULL", fn);
    if (mode != TVR_MESH_CROSSINGS_SELF && mode != TVR_MESH_CROSSINGS_MESH)
        return fail(TVR_ERR_INVALID, "%s: mode = %d is neither 0 (self query) nor 1 (two-mesh query)", fn, (int)mode);
    if (mode == TVR_MESH_CROSSINGS_MESH) {
        if (n_triangles_q < 0 || n_vertices_q < 0)
            return fail(TVR_ERR_INVALID, "%s: n_triangles_q = %lld / n_vertices_q = %lld is negative", fn, (long long)n_triangles_q, (long long)n_vertices_q);
        if (n_triangles_q > TVR_MESH_BVH_MAX_TRIANGLES)
            return fail(TVR_ERR_UNSUPPORTED, "%s: n_triangles_q = %lld: at most TVR_MESH_BVH_MAX_TRIANGLES = %d", fn, (long long)n_triangles_q, TVR_MESH_BVH_MAX_TRIANGLES);
        if ((rc = count_check(fn, "n_vertices_q", n_vertices_q, INT32_MAX, "vertex indices are int32")) != TVR_OK) return rc;
        if (n_triangles_q > 0 && (!faces_q || !verts_q)) return fail(TVR_ERR_INVALID, "%s: faces_q / verts_q is NULL with %lld query triangles", fn, (long long)n_triangles_q);
    }
    return bvh_blob(fn, bvh, bvh_bytes, n_triangles);
}

int tvr_mesh_crossings_count(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, int32_t mode,
                             const float *verts_q, int64_t n_vertices_q, const int32_t *faces_q, int64_t n_triangles_q, int32_t *count_out, size_t count_bytes,
                             int64_t *total_dev, int64_t *counts_dev, uint32_t *fault_flag_dev, void *stream)
{
    int rc = crossings_args(__func__, verts, n_vertices, faces, n_triangles, bvh, bvh_bytes, mode, verts_q, n_vertices_q, faces_q, n_triangles_q, fault_flag_dev);
    if (rc != TVR_OK) return rc;
    const int self = mode == TVR_MESH_CROSSINGS_SELF;
    const int64_t nq = self ? n_triangles : n_triangles_q;
    if (!total_dev) return fail(TVR_ERR_INVALID, "%s: total_dev is NULL", __func__);
    if (nq > 0 && !count_out) return fail(TVR_ERR_INVALID, "%s: count_out is NULL with %lld query triangles", __func__, (long long)nq);
    if ((rc = out_check(__func__, "count_out", count_bytes, nq, 0, 4, "query triangles x int32", TVR_ERR_SCRATCH)) != TVR_OK) return rc;
    HIP_TRY(launch_mesh_crossings_count(verts, n_vertices, faces, n_triangles, bvh, verts_q, n_vertices_q, faces_q, n_triangles_q, self, count_out,
                                        (unsigned long long *)total_dev, (unsigned long long *)counts_dev, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}

int tvr_mesh_crossings_emit(const float *verts, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const void *bvh, size_t bvh_bytes, int32_t mode,
                            const float *verts_q, int64_t n_vertices_q, const int32_t *faces_q, int64_t n_triangles_q, const int64_t *offsets, size_t offsets_bytes,
                            int64_t n_pairs, int32_t *pairs, size_t pairs_bytes, int32_t *n_pierce, size_t n_pierce_bytes, float *points, size_t points_bytes,
                            uint32_t *fault_flag_dev, void *stream)
{
    int rc = crossings_args(__func__, verts, n_vertices, faces, n_triangles, bvh, bvh_bytes, mode, verts_q, n_vertices_q, faces_q, n_triangles_q, fault_flag_dev);
    if (rc != TVR_OK) return rc;
    const int self = mode == TVR_MESH_CROSSINGS_SELF;
    const int64_t nq = self ? n_triangles : n_triangles_q;
    if ((rc = count_check(__func__, "n_pairs", n_pairs, INT32_MAX, "at most 2^31 - 1 pairs per call")) != TVR_OK) return rc;
    if (nq > 0 && !offsets) return fail(TVR_ERR_INVALID, "%s: offsets is NULL with %lld query triangles", __func__, (long long)nq);
    if ((uintptr_t)offsets % 8) return fail(TVR_ERR_INVALID, "%s: offsets is not 8-byte aligned", __func__);
    if (nq > 0 && (rc = out_check(__func__, "offsets", offsets_bytes, nq, 1, 8, "query triangles + 1 x int64", TVR_ERR_SCRATCH)) != TVR_OK) return rc;
    if (n_pairs > 0 && (!pairs || !n_pierce)) return fail(TVR_ERR_INVALID, "%s: pairs / n_pierce is NULL with %lld pairs", __func__, (long long)n_pairs);
    NEED("pairs [n_pairs,2]", pairs_bytes, n_pairs, 2);
    NEED("n_pierce [n_pairs]", n_pierce_bytes, n_pairs, 1);
    if (points) NEED("points [n_pairs,2,3]", points_bytes, n_pairs, 6);
    HIP_TRY(launch_mesh_crossings_emit(verts, n_vertices, faces, n_triangles, bvh, verts_q, n_vertices_q, faces_q, n_triangles_q, self, (const long long *)offsets, n_pairs,
                                       pairs, n_pierce, points, fault_flag_dev, (hipStream_t)stream));
    return TVR_OK;
}
