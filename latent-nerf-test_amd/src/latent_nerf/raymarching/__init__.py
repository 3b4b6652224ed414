from .raymarching import (MarchResult, bake_view_poses, chart_atlas, clean_mesh, compact_rays, composite_rays, composite_rays_train,
                          decimate_mesh, distortion_loss, gaussian_taps, get_rays, image_smooth, march_rays, march_rays_train,
                          marching_cubes, mesh_components, mesh_filter, mipcov_pull, mipcov_pull_backward, mipcov_push,
                          mipcov_weights, morton3D, morton3D_invert, near_far_from_aabb,
                          nerf_camera_record, normal_image, packbits, project_views, project_views_bands, pull_push_fill, smooth_mesh, uv_dilate, uv_raster,
                          view_lowpass, view_overlap_stats, view_zbuffer)

__all__ = ["MarchResult", "bake_view_poses", "chart_atlas", "clean_mesh", "compact_rays", "composite_rays", "composite_rays_train",
           "decimate_mesh", "distortion_loss", "gaussian_taps", "get_rays", "image_smooth", "march_rays", "march_rays_train",
           "marching_cubes", "mesh_components", "mesh_filter", "mipcov_pull", "mipcov_pull_backward", "mipcov_push",
           "mipcov_weights", "morton3D", "morton3D_invert", "near_far_from_aabb",
           "nerf_camera_record", "normal_image", "packbits", "project_views", "project_views_bands", "pull_push_fill", "smooth_mesh", "uv_dilate", "uv_raster",
           "view_lowpass", "view_overlap_stats", "view_zbuffer"]
