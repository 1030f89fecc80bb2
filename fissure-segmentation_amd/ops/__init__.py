"""The stateless op families behind `functional`: mesh, shape-model, volume, bit-plane, grid and voxel-CNN wrappers.  Each
module imports `_launch`, `_lib` and other ops modules only, never `functional`, and keeps no module-level switch; callers
go through `functional`, which re-exports every public name.  `labelmap_distances` / `_quantile_linear` (`metrics`) and
`mesh_remove_vertices` (`mesh.Meshes`) import their module inside the function, as they always did: both modules import
`functional`, so they cannot be imported while this package loads."""
