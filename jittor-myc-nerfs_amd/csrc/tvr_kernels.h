// tvr_kernels.h — host-visible launcher declarations shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/tvr.h"

struct SceneDev;

// records the text tvr_last_error() returns (thread-local) and hands `code` back; defined in tvr_api.hip
int tvr_set_error(int code, const char *fmt, ...);

// a HIP call inside a function that returns a status: its failure becomes TVR_ERR_HIP with the call's text and HIP's message
#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return tvr_set_error(TVR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Outputs of the march kernel / inputs of shade + composite.  The "queue" holds one entry per appearance sample
// (weight > thres); each ray's entries are contiguous and in sample order.
struct MarchOut {
    unsigned *counter;        // queue length (zeroed by the host before the march)
    unsigned *ray_off;        // [n_rays] first entry of the ray
    unsigned *ray_cnt;        // [n_rays] entries of the ray
    float *acc;               // [n_rays] sum of ALL weights (tensorBase.py:520)
    float *depth;             // [n_rays] final depth_map (written by the march kernel)
    float4 *q_pos;            // [cap] {xyz_norm, weight}
    float4 *q_out;            // [cap] {rgb, weight} written by the shade kernel (may alias q_pos)
    unsigned *q_ray;          // [cap] ray index (for the view direction)
    unsigned *q_j;            // [cap] sample index, or nullptr
    unsigned long long *stats;// TVR_STAT_* counters or nullptr
    float *lam6;              // [n_rays] prod_j (1 - alpha_j + 1e-6) (NerfPlusPlus bg_lambda, nerfplusplus.py:277-278) or nullptr
};

// how the samples of a ray are placed: uniform steps from the box entry (+ one jitter per ray), or explicit depths [n,S]
struct MarchSampling {
    const float *jitter;      // [n_rays] or nullptr
    const float *zv;          // [n_rays,S] or nullptr (NerfPlusPlus.sample_ray, nerfplusplus.py:239-269)
};

// a CP scene (TensorCP, models/tensoRF.py:317-447) beside its SceneDev: the lines sit where SceneDev has the VM lines (dline[i] / aline[i], line i along axis 2 - i),
// packed [L+1][rd] / [L+1][ra] fp32 (zero pad texel at index L, zero pad channels); SceneDev itself is unchanged, so no existing kernel's arguments move
struct CpDev {
    int rd, ra;               // channels per packed texel: density components rounded up to 16, appearance components rounded up to 4
    const float4 *basis;      // basis_mat [27, R_app] as [ra / 4][27] float4: entry (g, c) holds columns 4 g .. 4 g + 3 of row c (zero behind R_app)
};

// packed (channels-last, zero-padded) gradient images of the VM factors, same geometry as the packed scene
struct TrainGrads {
    float *dplane[3], *dline[3], *aplane[3], *aline[3];
};

enum { SH_SRC_QUEUE = 0, SH_SRC_XYZ = 1, SH_SRC_FEAT = 2, SH_SRC_H = 3 };       // SRC_H: h [n,144] given (training forward)
enum { SH_DST_QUEUE = 0, SH_DST_FEAT = 1, SH_DST_RGB = 2, SH_DST_TRAIN = 3 };    // DST_TRAIN: rgb + the activations the backward needs

struct ShadeArgs {
    const unsigned *counter;   // SRC_QUEUE: entry count lives on the device
    long long n;               // other modes: entry count
    float4 *q_pos;
    float4 *q_out;
    const unsigned *q_ray;
    const float *rays;         // [n_rays,6]
    const float *xyz;          // SRC_XYZ: xyz_norm [n,3]
    const float *viewdirs;     // SRC_FEAT: [n,3]
    const float *feats;        // SRC_FEAT: [n,27]
    float *out;                // DST_FEAT [n,27] / DST_RGB [n,3]
    const float *dots;         // REFTensoRF, SRC_FEAT: the dot_product input of MLPRender_Fea_Ref [n]
    float *out2;               // REFTensoRF, DST_FEAT: [n,8] {normal 3, rgb_d 3, specular_tint, rho}
    const float *h_in;         // SRC_H: h [n,144] (tvr_app_h_forward)
    float *t_feats, *t_h1, *t_h2;   // DST_TRAIN: features [n,32] (27 + zero pad), relu(layer 1) [n,128], relu(layer 2) [n,128]
    float *t_g8, *t_rgbs;           // DST_TRAIN, REFTensoRF: raw head outputs [n,8] {normal 3, tint, rgb_d 3, rho}, the MLP's sigmoid output [n,3]
    unsigned long long *stats;
};

// dvol: the scene's baked density volume (tvr_scene_set_density_volume, baked by launch_density_volume) or nullptr — the render entries pass it, the training forward
// keeps the factored evaluation
hipError_t launch_march(const SceneDev &sc, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T,
                        const MarchOut &mo, const tvr_dense_out *dense, hipStream_t stream, const float *dvol = nullptr);
hipError_t launch_density_volume(const SceneDev &sc, float *out, hipStream_t stream);
hipError_t launch_composite(const MarchOut &mo, int n_rays, int white_bg, float *rgb, hipStream_t stream);
hipError_t launch_scatter_rgb(const MarchOut &mo, int S, float *rgb_dense, hipStream_t stream);
hipError_t launch_density_feature(const SceneDev &sc, const float *xyz, long long m, float *out, hipStream_t stream);
// symmetric-difference gradient of launch_density_feature's value: grad [m,3] = (f(p + h e_k) - f(p - h e_k)) * inv2h[k]; sigma_feature [m] or nullptr receives f(p)
hipError_t launch_density_gradient(const SceneDev &sc, const float *xyz, long long m, const float h[3], const float inv2h[3], float *sigma_feature, float *grad,
                                   hipStream_t stream);
hipError_t launch_alpha_sample(const SceneDev &sc, const float *xyz, long long m, float *out, hipStream_t stream);
// fvol: the scene's baked appearance volume (tvr_scene_set_appearance_volume, baked by launch_appearance_volume) or nullptr — only the render path's kernel on 16x16x32
// tiles (queue -> queue, default arithmetic) reads it; every other mode evaluates the factored form
hipError_t launch_shade(const SceneDev &sc, int src, int dst, const ShadeArgs &a, hipStream_t stream, const float4 *fvol = nullptr);
// tvr_shade16.hip: the render path (queue -> queue, TensorVMSplit, default arithmetic, at most two encoding frequencies) on 16x16x32 tiles, and its fragment images
hipError_t launch_shade16(const SceneDev &sc, const ShadeArgs &a, hipStream_t stream, const float4 *fvol = nullptr);
hipError_t launch_appearance_volume(const SceneDev &sc, void *out, hipStream_t stream);
struct MlpShape;
hipError_t launch_pack16(const float *W1, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3, const float *basis, void *img, void *basg,
                         const MlpShape &sh, hipStream_t stream, const float *const *ref_W = nullptr, const float *const *ref_b = nullptr, void *refg = nullptr);
hipError_t launch_pack_plane(const float *in, float *out, int Cin, int C, int H, int W, hipStream_t stream);
// the scene's MLP_Fea / basis shape as the reference holds it (<= the shape the kernels are built for; packed with zero padding)
struct MlpShape {
    int featureC, fea_pe, view_pe, n_in;          // n_in = 30 + 54 fea_pe + 6 view_pe (+ 1 for REFTensoRF)
    int app_n_comp[3], app_off[3], k_app;         // basis_mat is [27][k_app], k_app = sum app_n_comp
};
hipError_t launch_pack_mlp(const float *W, const float *bias, void *out_hi, void *out_lo, int mode, const MlpShape &sh, hipStream_t stream);
hipError_t launch_pack_ref(const float *const W[4], const float *const b[4], void *rows, float *bias, hipStream_t stream);
hipError_t launch_march_backward(const SceneDev &sc, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                                 const float *grad_w, const float *grad_acc, const float *lam6, const float *grad_lam6, const TrainGrads &tg,
                                 hipStream_t stream, long long gw_cap = -1);    // gw_cap >= 0: grad_w holds gw_cap entries; a step whose queue is longer (or faulted) scatters nothing
// xyz_stride: 3 (xyz [m,3]) or 4 (the march queue's {xyz, w}); m_dev: optional device-side entry count, m is then the capacity (min of the two is processed)
hipError_t launch_app_h_forward(const SceneDev &sc, const float *xyz, long long m, float *h, hipStream_t stream, int xyz_stride = 3, const unsigned *m_dev = nullptr);
hipError_t launch_app_h_backward(const SceneDev &sc, const float *xyz, long long m, const float *dh, const TrainGrads &tg, hipStream_t stream, int xyz_stride = 3,
                                 const unsigned *m_dev = nullptr);
hipError_t launch_unpack_grad(const float *in, float *out, int Cout, int C, int H, int W, hipStream_t stream);
// m_dev: optional device-side row count; M is then the capacity (the grid is sized for it, the slabs are cut from min(*m_dev, M) on the device)
hipError_t launch_gemm_tn(const float *A, int lda, int Ka, const float *B, int ldb, int Kb, long long M, float *C, float *scratch, hipStream_t stream,
                          const unsigned *m_dev = nullptr, float *bias_out = nullptr,       // bias_out [Ka]: also the column sums of A (scratch sized for Kb + 1)
                          const float *scale_f16 = nullptr);   // device scalar s (a power of two): products on the fp16-split MFMAs with A * s (operands known to fit fp16 at that scale)
size_t gemm_tn_scratch_bytes(int Ka, int Kb, long long M);
hipError_t launch_pe_concat(const float *feat, const float *dir, const float *dot, long long m, float *X, hipStream_t stream);
hipError_t launch_pe_concat_strided(const float *feat, int fs, const float *dir, int ds, const float *rays, const unsigned *q_ray, const float *dot, int dts,
                                    long long m_cap, const unsigned *m_dev, float *X, hipStream_t stream);
hipError_t launch_pe_concat_backward(const float *feat, const float *dir, const float *gX, long long m, int with_dot, float *gfeat, float *gdir,
                                     float *gdot, hipStream_t stream);
// more than two encoding frequencies: X as column blocks of TVR_GENX_W columns, block b a contiguous [m_cap, w_b] matrix at X + b * m_cap * TVR_GENX_W (tvr_train.hip)
#define TVR_GENX_W 152
#define TVR_GENX_FLOATS (3 * TVR_GENX_W)          // per entry, at most: 390 columns = 152 + 152 + 88
hipError_t launch_pe_concat_gen(const float *feat, int fs, const float *rays, const unsigned *q_ray, int fea_pe, int view_pe, long long m_cap, const unsigned *m_dev, float *X,
                                hipStream_t stream);
hipError_t launch_copy_cols(float *dst, int ldd, int col0, const float *src, int lds, int ncols, int nrows, hipStream_t stream);
size_t mlp_train_image_bytes();
// heads: REFTensoRF's {normal [3,144], diffuse [3,144], specular [1,144], rho [1,144]} weights, or nullptr (TensorVMSplit)
// fea_pe / view_pe > 2 (TensorVMSplit only): W1 is [128, 30 + 54 fea_pe + 6 view_pe] and is packed into the streamed image behind the LDS image (tvr_mlp_train.hip, TI_W1G)
hipError_t launch_pack_train_image(const float *W1, const float *W2, const float *W3, const float *Bas, const float *const heads[4], void *image, hipStream_t stream,
                                   int fea_pe = 2, int view_pe = 2, const int *app_n_comp = nullptr,      // app_n_comp[3] <= 48 each (nullptr: 48): basis is [27, sum app_n_comp]
                                   int featureC = 128);                                                    // <= 128: W1 [fc, n_in], W2 [fc, fc], W3 [3, fc]
// REFTensoRF's additions to the backward: raw head outputs, view directions, optional gradient of the -dot output; dg8 [m,8] is written
struct MlpRefBwd { const float *g8, *viewdirs, *grad_in0; float *dg8; const float *rays; const unsigned *q_ray; };   // q_ray set: the direction of entry e is rays[q_ray[e]][3..5]
hipError_t launch_mlp_train_backward(const float *grad_rgb, const float *rgb, const float *feats, const float *h1, const float *h2, long long m, const float *gscale,
                                     float *d_out, float *dh2, float *dh1, float *dfeats, float *dh, unsigned *sat_flag, void *image, const MlpRefBwd *ref,
                                     hipStream_t stream, const unsigned *m_dev = nullptr, int gen = 0);
// up to 8 parameter tensors of a regulariser (tvr_reg.hip): x / grad pointers, element counts, rows (line factors: n_comp), launch blocks
#define TVR_REG_MAX 8
struct RegList {
    const float *x[TVR_REG_MAX];
    float *grad[TVR_REG_MAX];
    long long count[TVR_REG_MAX];
    int rows[TVR_REG_MAX];
    int blocks[TVR_REG_MAX];
    int n;
};
size_t reg_l1_scratch_bytes(const RegList &L);
hipError_t launch_l1_forward(const RegList &L, float *value, float *scratch, hipStream_t stream);
hipError_t launch_l1_backward(const RegList &L, const float *g, hipStream_t stream);
hipError_t launch_ortho(const RegList &L, const float *g, float *value, float *scratch, hipStream_t stream);
hipError_t launch_tv_loss(const float *x, int C, int H, int W, float weight, float *value, float *grad, float *part, hipStream_t stream);
hipError_t launch_alpha_bits(const float *vol, long long n, unsigned *bits, hipStream_t stream);

// tvr_step.hip: the training step's compositing tail (forward / backward over the queue, device-side counts), gradient scale, column sums
hipError_t launch_composite_train_forward(const MarchOut &mo, int n_rays, long long cap, int white_bg, const float *rgb, const float *feats32, int with_pen, float *rgb_map,
                                          float *pre, float *pen_ray, hipStream_t stream);
hipError_t launch_composite_train_backward(const MarchOut &mo, int n_rays, long long cap, int white_bg, const float *rgb, const float *feats32, const float *g8, const float *pre,
                                           const float *g_map, const float *g_pen, float *grgb, float *gin0, float *grad_w, float *grad_acc, unsigned *amax_bits,
                                           float target, float *gscale, hipStream_t stream);
// the march queue of a training batch put into RAY ORDER (scan of the per-ray counts, gather into tmp_pos / tmp_ray, copy back; ray_off is updated)
hipError_t launch_queue_ray_order(const MarchOut &mo, unsigned *ray_new, float4 *tmp_pos, unsigned *tmp_ray, int n_rays, hipStream_t stream);
hipError_t launch_linear_dx(const float *dY, int ldy, int N, const float *W, int ldw, int n_valid, int K, const float *mask, int ldm, float *dX, int ldx, long long M,
                            hipStream_t stream, const float *scale = nullptr, unsigned *sat_flag = nullptr, const unsigned long long *mask_bits = nullptr);
hipError_t launch_filter_rays(const SceneDev &sc, const float *rays, long long n, int S, int bbox_only, unsigned char *mask, hipStream_t stream);
size_t colsum_scratch_bytes();
hipError_t launch_colsum(const float *A, int lda, int K, long long m_cap, const unsigned *m_dev, float *out, float *scratch, hipStream_t stream);
hipError_t launch_copy_f32(float *dst, const float *src, int n, hipStream_t stream);
hipError_t launch_zero_header(unsigned *counter, hipStream_t stream);
hipError_t launch_f32_to_f16(const float *in, void *out, long long n, hipStream_t stream);      // n a multiple of 4; round to nearest even
hipError_t launch_zero_f32(float *p, long long n, hipStream_t stream);

// tvr_cp.hip: the CP field's own kernels.  launch_cp_march has launch_march's contract; launch_cp_app_feature writes features [m,27] for xyz [m, xyz_stride]
// (m_dev: optional device-side count, m is then the capacity) and, with q_ray / rays given, the entries' view directions dirs [m,3];
// launch_cp_rgbw carries rgb [cap,3] and the queue's weights into q_out for composite_kernel / scatter_rgb_kernel (and counts the appearance samples into stats)
hipError_t launch_cp_march(const SceneDev &sc, const CpDev &cp, const float *rays, int n_rays, int S, const MarchSampling &sm, float eps_T, const MarchOut &mo,
                           const tvr_dense_out *dense, hipStream_t stream);
hipError_t launch_cp_density_feature(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, float *out, hipStream_t stream);
hipError_t launch_cp_density_gradient(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, const float h[3], const float inv2h[3], float *sigma_feature,
                                      float *grad, hipStream_t stream);
hipError_t launch_cp_app_feature(const SceneDev &sc, const CpDev &cp, const float *xyz, int xyz_stride, long long m, const unsigned *m_dev, const unsigned *q_ray,
                                 const float *rays, float *feats, float *dirs, hipStream_t stream);
hipError_t launch_cp_rgbw(const MarchOut &mo, const float *rgb, long long cap, hipStream_t stream);
// tvr_cp_train.hip: the CP field's backward kernels.  gline[i]: the packed gradient image of line i ([L_i + 1][rd] / [L_i + 1][ra] fp32, zeroed by the caller); gbasis:
// [27][ra] fp32, zeroed by the caller; xyz [m,3], dF [m,27].  Sums are float atomics: reproducible to rounding.
hipError_t launch_cp_march_backward(const SceneDev &sc, const CpDev &cp, const float *rays, int n_rays, int S, const float *jitter, float eps_T, const MarchOut &mo,
                                    const float *grad_w, const float *grad_acc, float *const gline[3], hipStream_t stream);
hipError_t launch_cp_app_backward(const SceneDev &sc, const CpDev &cp, const float *xyz, long long m, const float *dF, float *const gline[3], float *gbasis,
                                  hipStream_t stream);
hipError_t launch_cp_pack_basis(const float *basis, int r_app, int ra, float4 *out, hipStream_t stream);
int march_cu_count();

// tvr_normals.hip: the march's queue -> normal [n,3] = sum over a ray's entries of weight x unit(-gradient of the density feature x inv_aabb_size); acc_out [n] or nullptr
// receives mo.acc, and with the march's fault flag set every output of the call (depth_out [n] or nullptr included) is NaN.  cp: the CP scene's part, or nullptr (VM).
// Draws its ray tickets from a word of the scratch header that launch_zero_header cleared in front of the march.
hipError_t launch_normals(const SceneDev &sc, const CpDev *cp, const MarchOut &mo, int n_rays, const float h[3], const float inv2h[3], float *normal_out, float *acc_out,
                          float *depth_out, hipStream_t stream);

// tvr_mesh.hip: marching cubes over a dense fp32 volume [nx][ny][nz] (z fastest).  The scratch buffer carved for a volume of `points` grid points: a header with the
// totals, per tile of TVR_MESH_TILE points its base (vertices | triangles << 32), per point one count byte and the two exclusive bases (arrays padded to whole tiles)
struct MeshScratch {
    unsigned long long *totals, *tile_base;
    unsigned char *cnt8;
    unsigned *vbase, *tbase;
    unsigned n_tiles;
    size_t total;
};
MeshScratch mesh_carve(long long points, void *scratch);
size_t mesh_scratch_bytes(long long points);
// count + scan: fills the scratch, leaves {vertices, triangles} in counts_dev[2]
hipError_t launch_mesh_count(const float *vol, const int dims[3], float level, const MeshScratch &s, long long *counts_dev, hipStream_t stream);
// the scan half of launch_mesh_count over a scratch whose cnt8 / tile_base are filled (also the component filter's, tvr_mesh_cc.hip): tile bases, totals -> counts_dev[2]
// and the scratch header, per-element bases
hipError_t launch_mesh_scan(const MeshScratch &s, long long *counts_dev, hipStream_t stream);
// emit from a filled scratch; n_vertices / n_triangles are the capacities of verts / faces AND must equal the counted totals, else *fault = 1 and nothing is written
hipError_t launch_mesh_emit(const float *vol, const int dims[3], float level, const float origin[3], const float spacing[3], const MeshScratch &s, float *verts,
                            long long n_vertices, int *faces, long long n_triangles, int flip, unsigned *fault, hipStream_t stream);

// tvr_mesh_cc.hip: connected components of an indexed triangle mesh (union-find over the vertices, the label array is the parent array) and the component filter.
// The components' scratch is one header of MESH_CC_SCRATCH_BYTES: {uint32 bad index seen, uint32 most steps of any walk}.  The filter's scratch is a MeshScratch over
// max(V, F) elements: count byte bit 0 = vertex kept, bit 3 = triangle kept (what the scan kernels read as one vertex / one triangle); totals[1] != 0 = bad input seen.
#define MESH_CC_SCRATCH_BYTES 256
hipError_t launch_mesh_components(const int *faces, long long n_triangles, long long n_vertices, int *vertex_label, int *component_faces, long long *n_components,
                                  void *scratch, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_filter_count(const int *faces, long long n_triangles, long long n_vertices, const int *vertex_label, const unsigned char *keep_root,
                                    const MeshScratch &s, long long *counts_dev, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_filter_emit(const float *verts, const int *faces, long long n_triangles, long long n_vertices, const MeshScratch &s, float *verts_out,
                                   long long n_vertices_out, int *faces_out, long long n_triangles_out, int *kept_vertex, unsigned *fault, hipStream_t stream);

// tvr_mesh_simplify.hip: vertex-clustering simplification of an indexed triangle mesh (include/tvr.h tvr_mesh_simplify_*).  The scratch carved for V vertices and
// F triangles: a header {uint32 bad input seen, uint32 longest probe sequence}, a MeshScratch over max(V, F) elements (count byte bit 0 = vertex e is its cluster's
// representative, bit 3 = triangle e survives: tvr_mesh.hip's scan reads them as one vertex / one triangle), per vertex its cluster's representative, per triangle its
// slot, the two hash tables (cells: 64-bit key + representative per slot; triangles: one triangle index per slot) and per vertex {members, sum qx, sum qy, sum qz}.
struct SimplifyScratch {
    unsigned *header;
    MeshScratch flags;
    unsigned *vrep;                    // [V] after the cell pass: the vertex's slot; after the resolve pass: its cluster's representative
    unsigned *tslot;                   // [F] the triangle's slot (0 for a collapsed triangle, which sits in no slot)
    unsigned long long *cell_key;      // [cap_v], empty = all ones
    unsigned *cell_rep;                // [cap_v], the smallest vertex index that reached the slot
    unsigned *tri_slot;                // [cap_t], the smallest triangle index of the slot's triple, empty = all ones
    unsigned long long *sums;          // [V][4], read at representatives
    unsigned long long cap_v, cap_t;   // powers of two, >= 2 V / 2 F
    size_t fill_off, fill_bytes;       // the tables: one 0xff fill before the count
    size_t sums_off, sums_bytes;       // zeroed before the emit
    size_t total;
};
struct SimplifyLattice {
    float origin[3], cell[3], inv_cell[3];
};
SimplifyScratch simplify_carve(long long n_vertices, long long n_triangles, void *scratch);
hipError_t launch_mesh_simplify_count(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const SimplifyLattice &lat,
                                      const SimplifyScratch &s, long long *counts_dev, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_simplify_emit(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const SimplifyLattice &lat,
                                     const SimplifyScratch &s, float *verts_out, long long n_vertices_out, int *faces_out, long long n_triangles_out, int *vertex_map,
                                     unsigned *fault, hipStream_t stream);

// tvr_mesh_smooth.hip: vertex adjacency of an indexed triangle mesh and Taubin smoothing over it (include/tvr.h tvr_mesh_adjacency_* / tvr_mesh_smooth).  The adjacency's
// scratch carved for V vertices and F triangles: a header {bad input seen, long rows, boundary edges, non-manifold edges, largest degree, H, raw entries}, the scan's
// tile sums, per vertex its degree (first the raw degree, then the fill's cursor, then the distinct neighbours) and a slot in the list of long rows, the raw row starts
// and the offsets (V + 1 each), and two arrays of 6 F entries: the raw rows (after the sort: each row's distinct neighbours at its front) and, parallel, edge_faces.
#define ADJ_SHORT TVR_MESH_ADJ_SHORT_ROW
struct AdjScratch {
    unsigned *header, *tile, *deg, *long_rows, *raw_off, *off, *raw, *cnt;
    unsigned raw_cap, n_tiles;
    size_t total;
};
AdjScratch adj_carve(long long n_vertices, long long n_triangles, void *scratch);
hipError_t launch_mesh_adjacency_count(const int *faces, long long n_triangles, long long n_vertices, const AdjScratch &s, long long *counts_dev, unsigned *fault,
                                       hipStream_t stream);
hipError_t launch_mesh_adjacency_emit(long long n_vertices, const AdjScratch &s, int *offsets, int *neighbours, int *edge_faces, long long n_half_edges, unsigned *fault,
                                      hipStream_t stream);
// the smoothing's scratch: a header {bad adjacency seen} and the two ping-pong buffers of 16-byte rows {x, y, z, pinned}
struct SmoothScratch {
    unsigned *header;
    float4 *rows[2];
    size_t total;
};
SmoothScratch smooth_carve(long long n_vertices, void *scratch);
hipError_t launch_mesh_smooth(const float *verts, long long n_vertices, const int *offsets, const int *neighbours, const int *edge_faces, long long n_half_edges,
                              int iterations, float lambda, float mu, const SmoothScratch &s, float *verts_out, unsigned *fault, hipStream_t stream);

// tvr_mesh_project.hip: Newton projection of vertices onto the iso-surface density feature == target_feature (include/tvr.h tvr_mesh_project).  cp: the scene's CpDev
// or nullptr (VM); h / inv2h: tvr_density_gradient's half width and 0.5 / h; pinned / residual_in may be nullptr; counts [4] must have been zeroed on `stream`.
hipError_t launch_mesh_project(const SceneDev &sc, const CpDev *cp, const float *verts, long long n_vertices, const unsigned char *pinned, float target_feature,
                               int iterations, const float h[3], const float inv2h[3], const float max_move[3], float tol, float *verts_out, float *residual_in,
                               float *residual_out, unsigned long long *counts, hipStream_t stream);

// tvr_mesh_raster.hip: the z-buffer rasteriser of indexed triangle meshes (include/tvr.h tvr_mesh_raster).  Scratch: a header of MESH_RASTER_HEADER_BYTES {uint32 bad
// index seen, uint32 queue length}, H*W 64-bit keys (depth bits << 32 | triangle), a queue of n_triangles int32 (triangles whose box exceeds large_bbox), each array
// rounded up to 256 B.
#define MESH_RASTER_HEADER_BYTES 256
size_t mesh_raster_scratch_bytes(long long n_triangles, long long n_pixels);
hipError_t launch_mesh_raster(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const tvr_mesh_camera &cam, const float *attr, int n_attr,
                              float *depth, int *tri, float *bary, float *attr_out, void *scratch, int *counts, unsigned *fault, hipStream_t stream);

// tvr_mesh_texture.hip: the per-triangle texture atlas (include/tvr.h tvr_mesh_atlas_points / tvr_mesh_texture_sample).  No scratch.  The host has checked the counts,
// the layout (Wa = C * P, fewer than 2^31 texels) and the range; n <= 0 / n_pix <= 0 launch nothing.  fmt 0: atlas uint8 [n_texels][3], 1: fp32.
hipError_t launch_mesh_atlas_points(const float *verts, long long n_vertices, const int *faces, long long n_triangles, int P, int C, long long texel0, long long n,
                                    float *pos, int *tri, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_texture_sample(const int *tri, const float *bary, long long n_pix, const void *atlas, int fmt, long long n_texels, int P, int C,
                                      long long n_triangles, float *out, hipStream_t stream);

// tvr_mesh_bvh.hip: the linear BVH over a mesh's triangles and its ray queries (include/tvr.h tvr_mesh_bvh_*).  The blob: a header of MESH_BVH_HEADER_BYTES, the boxes
// of the 2F-1 nodes (internal nodes 0 .. F-2, then the leaves in key order; 6 fp32 each), the F-1 child pairs, the F triangle indices of the leaves, each array rounded
// up to 256 B.  The build's scratch: 256 B of header, one pass word per internal node, one bit per triangle.  The host has checked counts, pointers, sizes and alignment.
#define MESH_BVH_HEADER_BYTES 256
struct MeshBvhCarve {
    size_t header, box, child, leaf_tri, total;
};
size_t mesh_bvh_bytes(long long n_triangles, MeshBvhCarve *carve);
size_t mesh_bvh_scratch_bytes(long long n_triangles);
hipError_t launch_mesh_bvh_keys(const float *verts, long long n_vertices, const int *faces, long long n_triangles, unsigned long long *keys, void *scratch, unsigned *fault,
                                hipStream_t stream);
hipError_t launch_mesh_bvh_build(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const unsigned long long *keys, void *bvh, void *scratch,
                                 int *counts, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_bvh_cast(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const float *origins, const float *dirs,
                                long long n_rays, float t_min, float t_max, int any_hit, int cull, float *t, int *tri, float *bary, unsigned char *hit,
                                unsigned long long *counts, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_bvh_nearest(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const float *points,
                                   long long n_points, float max_dist, float *dist, int *tri, float *bary, unsigned long long *counts, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_bvh_occlusion(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const float *points,
                                     const float *normals, long long n_points, const float *dirs, int n_dirs, float bias, float t_max, float *out, unsigned long long *counts,
                                     unsigned *fault, hipStream_t stream);

// tvr_mesh_pseudo.hip: the pseudo-normal table of a mesh (include/tvr.h tvr_mesh_pseudonormals_*), read by tvr_mesh_bvh.hip's signed query.  The blob: a
// header of MESH_PSEUDO_HEADER_BYTES, face_n [F][3], edge_n [F][3][3], vert_n [V][3] fp32, each array rounded up to 256 B.  The build's scratch: 256 B of header, one bit
// per corner, one bit per half-edge.  The host has checked counts, pointers, sizes and alignment.
#define MESH_PSEUDO_HEADER_BYTES 256
#define MESH_PSEUDO_MAGIC 0x4e505654u
struct MeshPseudoHeader {               // at the blob's start
    unsigned magic, F, V, bad, degenerate_faces, open_edges, nonmanifold_edges, inconsistent_edges;
};
struct MeshPseudoCarve {
    size_t header, face_n, edge_n, vert_n, total;
};
size_t mesh_pseudo_bytes(long long n_vertices, long long n_triangles, MeshPseudoCarve *carve);
size_t mesh_pseudo_scratch_bytes(long long n_triangles);
hipError_t launch_mesh_pseudo_keys(const int *faces, long long n_vertices, long long n_triangles, unsigned long long *corner_keys, unsigned long long *edge_keys,
                                   unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_pseudo_build(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const unsigned long long *corner_keys,
                                    const unsigned long long *edge_keys, const long long *edge_order, void *table, void *scratch, int *counts, unsigned *fault,
                                    hipStream_t stream);
// the signed query: points == nullptr selects the lattice (origin, spacing, dims; n_points = dims[0] * dims[1] * dims[2]); tri, bary and feature may be nullptr
hipError_t launch_mesh_bvh_signed(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const void *table, const float *points,
                                  const float *origin, const float *spacing, const int *dims, long long n_points, float max_dist, float *sdist, int *tri, float *bary,
                                  signed char *feature, unsigned long long *counts, unsigned *fault, hipStream_t stream);

// tvr_mesh_winding.hip: the table of node moments beside a hierarchy and the winding-number query (include/tvr.h tvr_mesh_winding_*).  The blob: a header
// of MESH_WINDING_HEADER_BYTES, then one row of 8 fp32 per internal node (A xyz, c xyz, r, a), rounded up to 256 B.  The build's scratch: one pass word and four fp32
// (the unnormalised moment) per internal node.  The host has checked counts, pointers, sizes and alignment.
#define MESH_WINDING_HEADER_BYTES 256
#define MESH_WINDING_MAGIC 0x4e575654u
struct MeshWindingHeader {              // at the blob's start
    unsigned magic, F, bad, reserved[5];
};
struct MeshWindingCarve {
    size_t header, rows, total;
};
size_t mesh_winding_bytes(long long n_triangles, MeshWindingCarve *carve);
size_t mesh_winding_scratch_bytes(long long n_triangles);
hipError_t launch_mesh_winding_build(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, void *table, void *scratch,
                                     unsigned *fault, hipStream_t stream);
// points == nullptr selects the lattice (origin, spacing, dims; n_points = dims[0] * dims[1] * dims[2])
hipError_t launch_mesh_winding_query(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const void *table,
                                     const float *points, const float *origin, const float *spacing, const int *dims, long long n_points, float beta, float *w,
                                     unsigned long long *counts, unsigned *fault, hipStream_t stream);

// tvr_mesh_crossings.hip: the triangle-pair query on a hierarchy (include/tvr.h tvr_mesh_crossings_*).  self != 0: the hierarchy's own mesh is the query
// (pairs i < j) and verts_q / faces_q are not read.  count: count_out [Fq], total [1], counts [4] or nullptr.  emit: offsets [Fq+1], pairs [n_pairs][2],
// n_pierce [n_pairs], points [n_pairs][2][3] or nullptr.  The host has checked counts, pointers, sizes and alignment.
hipError_t launch_mesh_crossings_count(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const float *verts_q,
                                       long long n_vertices_q, const int *faces_q, long long n_triangles_q, int self, int *count_out, unsigned long long *total,
                                       unsigned long long *counts, unsigned *fault, hipStream_t stream);
hipError_t launch_mesh_crossings_emit(const float *verts, long long n_vertices, const int *faces, long long n_triangles, const void *bvh, const float *verts_q,
                                      long long n_vertices_q, const int *faces_q, long long n_triangles_q, int self, const long long *offsets, long long n_pairs,
                                      int *pairs, int *n_pierce, float *points, unsigned *fault, hipStream_t stream);

