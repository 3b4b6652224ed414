from .raymarching import (MarchResult, chart_atlas, clean_mesh, compact_rays, composite_rays, composite_rays_train,
                          decimate_mesh, distortion_loss, get_rays, image_smooth, march_rays, march_rays_train,
                          marching_cubes, mesh_components, mesh_filter, morton3D, morton3D_invert, near_far_from_aabb,
                          normal_image, packbits, smooth_mesh, uv_dilate, uv_raster)

__all__ = ["MarchResult", "chart_atlas", "clean_mesh", "compact_rays", "composite_rays", "composite_rays_train",
           "decimate_mesh", "distortion_loss", "get_rays", "image_smooth", "march_rays", "march_rays_train",
           "marching_cubes", "mesh_components", "mesh_filter", "morton3D", "morton3D_invert", "near_far_from_aabb",
           "normal_image", "packbits", "smooth_mesh", "uv_dilate", "uv_raster"]
