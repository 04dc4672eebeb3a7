"""MI355X-native TensoRF volume renderer (package dir: jittor-myc-nerfs_amd; import as jittor_myc_nerfs_amd).

Drop-in surface of the reference's render path (tensorf-myc): TensorVMSplit / AlphaGridMask / MLPRender_Fea
(field.py), REFTensoRF / NerfPlusPlus (variants.py), OctreeRender_trilinear_fast (render.py), Blender-format ray generation (rays.py), backed by
hand-written HIP kernels for gfx950 behind the C-ABI in include/tvr.h (csrc/, built into lib/libtvr.so)."""
from .field import AlphaGridMask, MLPRender_Fea, TensorBase, TensorVMSplit, load_checkpoint  # noqa: F401
from .cp import TensorCP  # noqa: F401
from .variants import Embedder, MLPNet, MLPRender_Fea_Ref, NerfPlusPlus, REFTensoRF  # noqa: F401
from .render import OctreeRender_trilinear_fast, N_to_reso, cal_n_samples, render_sharded, ShardedFramePipeline, FrameStream, shard_indices, shard_capacity, shard_gather_index, shard_send_views, shard_unpermute  # noqa: F401
from .evaluation import BlenderRays, evaluation, evaluation_mesh, evaluation_path, mesh_agreement, normal_map_to_rgb8, rgb_ssim, rgb_ssim_torch  # noqa: F401
from .losses import TVLoss  # noqa: F401
from .mesh import marching_cubes, mesh_adjacency, mesh_view_to_rgb8, read_ply, read_ply_attributes, render_mesh, render_mesh_frame, simplify_clustering, smooth_taubin, write_ply  # noqa: F401
from .mesh import atlas_points, atlas_shape, atlas_uv, read_obj, sample_texture, write_obj  # noqa: F401
from .mesh import MeshBVH, ambient_occlusion, build_bvh, cast_rays, fibonacci_sphere  # noqa: F401
from .mesh import closest_points, mesh_distance, surface_samples  # noqa: F401
from .mesh import build_pseudonormals, contains, signed_distance, signed_distance_grid, signed_mesh_distance  # noqa: F401
from .mesh import build_winding, remesh_watertight, signed_distance_winding, winding_contains, winding_number, winding_number_grid  # noqa: F401
from .mesh import crossing_faces, mesh_check, mesh_intersections, self_intersections, write_obj_segments  # noqa: F401
from .training import GradBucket, make_graphed_step, shard_batch  # noqa: F401
from . import mesh, ngp, rays, synthetic  # noqa: F401
