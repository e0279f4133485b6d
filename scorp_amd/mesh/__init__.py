"""From a trained surfel model to a coloured triangle mesh: gs2dgs/utils/mesh_utils.py's GaussianExtractor
(reconstruction, estimate_bounding_sphere, extract_mesh_unbounded / compute_unbounded_tsdf) and the lattice of
gs2dgs/utils/mcube_utils.py, on the GPU.

    ex = GaussianExtractor(gaussians, render, pipe)
    ex.reconstruction(cameras)
    write_mesh_ply("mesh.ply", post_process_mesh(ex.extract_mesh_unbounded(resolution=512), cluster_to_keep=50))

The depth and colour maps stay on the device as two stacked tensors.  The TSDF of every sample is fused over all views by
one launch (csrc/tsdf.hip: scorp_tsdf_fuse), the volume is ONE dense grid (no 512^3 crops, so no crop seams and no
restriction of `resolution` to multiples of 512), and the surface is extracted by surface nets (csrc/isosurface.hip: one
vertex per cell the surface crosses, which lies in the same cell as the marching-cubes vertices of that cell) or, with
method="marching_cubes", by marching cubes (csrc/marching_cubes.hip: one vertex per crossed lattice edge, the triangles
from the case table that scorp_amd/mc_table.py generates).  `post_process_mesh` (mesh_utils.py:22-43) drops the floaters: the triangles are clustered over shared edges
by a lock-free union-find on the device (csrc/mesh_cluster.hip, Open3D's cluster_connected_triangles), the largest
clusters are kept and the mesh is compacted with torch ops, without a mesh-sized array visiting the host.
`extract_mesh_bounded`, the route the 2DGS paper reports its meshes with, fuses the same maps into a SPARSE volume instead:
16^3-voxel blocks that exist only within sdf_trunc of an observed depth point (csrc/tsdf_blocks.hip: a hashed block set, one
workgroup per block with the view loop inside), meshed by surface nets whose corner fetch goes through a block-neighbour table
(csrc/isosurface_blocks.hip) or by marching cubes that does (csrc/marching_cubes_blocks.hip).  The reference hands this to
Open3D's ScalableTSDFVolume and its marching cubes; the volume here
follows the rules written down in include/scorp_gs.h and was never compared with Open3D's own output, which was not
available.  `simplify_vertex_clustering` reduces the mesh: the vertices in one cell of a grid become one vertex, at their mean
or at the minimiser of the cell's plane quadrics (csrc/mesh_simplify.hip; the rules are this project's own, in
include/scorp_gs.h, uncompared with Open3D's simplify_vertex_clustering).  `simplify_quadric_decimation` reduces it to a
target triangle count by edge collapses, an independent set of edges per round (csrc/mesh_decimate.hip; again this
project's own rules, in include/scorp_gs.h).  `point_mesh_distance`, `sample_points_uniformly`, `nearest_point_distance`
and the figures of `mesh_distance` / `mesh_cloud_distance` MEASURE a mesh: the exact distance to the nearest triangle through a
uniform grid of (cell, triangle) pairs, in float64 (csrc/mesh_distance.hip; held to a float64 brute force of another
formulation, tests/mesh_distance_reference.py).  `render_mesh`, `face_visibility`, `cull_unseen_faces` and `depth_difference`
LOOK at a mesh from cameras: a z-buffer rasterizer with exact integer coverage and one 64-bit atomic minimum per candidate
(csrc/mesh_render.hip; this project's own rules, held to exact integers and fractions by tests/mesh_render_reference.py).
`filter_smooth_laplacian`, `filter_smooth_taubin`, `face_normals`, `vertex_normals`, `normal_map` and `normal_difference`
SMOOTH a mesh and give it normals: `mesh_adjacency` puts each vertex's neighbours and incident faces into CSR form in
ascending order, and one thread per vertex sums over its slice in float64, so the results are the same bits on every run
(csrc/mesh_smooth.hip; this project's own rules, in include/scorp_gs.h, held bit for bit to the per-vertex Python loops of
tests/mesh_smooth_reference.py; uncompared with Open3D's filters of the same names).

CUDA tensors run the HIP kernels; CPU tensors run a torch / numpy form of the same statements.

One module per subsystem, every public name re-exported here:
    _common.py    Mesh, empty_mesh, drop_unreferenced, check_mesh (the simplifiers' argument checks), METHODS
    _topology.py  edge_keys, vertex_face_csr, table_slots, proper_faces and the float64 numpy cross / dot / unit of the CPU forms
    tsdf.py       tsdf_fuse over samples or a lattice, uncontract
    surface.py    extract_surface: dense surface nets and marching cubes
    blocks.py     BlockVolume, tsdf_blocks_fuse, block_neighbors, extract_surface_blocks
    cluster.py    cluster_connected_triangles, post_process_mesh
    simplify.py   cluster_vertices, simplify_vertex_clustering
    decimate.py   simplify_quadric_decimation and its host loop _decimate over _DecimateHip / _DecimateNumpy
    distance.py   point_mesh_distance, sample_points_uniformly, nearest_point_distance, mesh_distance, mesh_cloud_distance
    render.py     render_mesh, face_visibility, cull_unseen_faces, depth_difference
    smooth.py     mesh_adjacency, face_normals, vertex_normals, filter_smooth_laplacian, filter_smooth_taubin, normal_map,
                  normal_difference
    extractor.py  focus_point, GaussianExtractor (imports the others; nothing imports it)
Every stream-taking C-ABI call of the package goes through _C.call.  A test that patches a module global (tsdf.LAUNCH_SAMPLES) patches the
home module: the names below are copies.
"""
from ._common import MAX_CLUSTER_FACES, MAX_SIMPLIFY_VERTICES, METHODS, Mesh, check_mesh, drop_unreferenced, empty_mesh
from .blocks import (BLOCK_SIDE, BLOCK_VOXELS, KEY_BIAS, MAX_TABLE_SLOTS, BlockVolume, block_coords, block_neighbors,
                     extract_surface_blocks, tsdf_blocks_fuse)
from .cluster import MIN_CLUSTER_TRIANGLES, _cluster_numpy, cluster_connected_triangles, post_process_mesh
from .decimate import DECIMATE_DET_FLOOR, DECIMATE_REACH, _decimate, _DecimateHip, simplify_quadric_decimation
from .distance import (MAX_CLOUD_POINTS, MAX_QUERIES, PAIR_CAP_FACTOR, PAIR_CAP_FLOOR, MeshDistance, NearestPoint, PointMeshDistance,
                       SurfaceSamples, mesh_cloud_distance, mesh_distance, nearest_point_distance, point_mesh_distance,
                       sample_points_uniformly, triangle_area_prefix)
from .extractor import GaussianExtractor, focus_point
from .render import (MAX_RENDER_SIDE, MAX_RENDER_VIEWS, WORKSPACE_CAP, DepthDifference, MeshRender, _render_mesh_numpy, cull_unseen_faces,
                     depth_difference, face_visibility, render_mesh)
from .simplify import CELL_SIDE, CONTRACTIONS, QUADRIC_TRUNCATE, cluster_vertices, simplify_vertex_clustering
from .smooth import (DISTANCE_EPS, MAX_SMOOTH_STEPS, SMOOTH_WEIGHTS, WEIGHTINGS, MeshAdjacency, NormalDifference, face_normals,
                     filter_smooth_laplacian, filter_smooth_taubin, mesh_adjacency, normal_difference, normal_map, vertex_normals)
from .surface import _scan_counts, _surface_nets_numpy, extract_surface
from .tsdf import LAUNCH_SAMPLES, MAX_RANGE, tsdf_fuse, uncontract
