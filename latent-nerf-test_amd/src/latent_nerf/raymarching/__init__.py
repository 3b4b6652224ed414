from .raymarching import (MarchResult, chart_atlas, compact_rays, composite_rays, composite_rays_train, decimate_mesh,
                          get_rays, march_rays, march_rays_train, marching_cubes, morton3D, morton3D_invert,
                          near_far_from_aabb, packbits, uv_dilate, uv_raster)

__all__ = ["MarchResult", "chart_atlas", "compact_rays", "composite_rays", "composite_rays_train", "decimate_mesh", "get_rays",
           "march_rays", "march_rays_train", "marching_cubes", "morton3D", "morton3D_invert", "near_far_from_aabb", "packbits",
           "uv_dilate", "uv_raster"]
