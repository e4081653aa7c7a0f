"""Drop-in for the two functions of `pytorch3d` that Texture-GS calls: `pytorch3d.loss.chamfer_distance`
(models/uv_map_gaussian3d.py:10, :205, :216) and `pytorch3d.ops.sample_farthest_points` (extract_pcd.py:5, :19) resolve to the HIP
implementations in texgs.uvmap and texgs.points when texture-gs_amd/ is on PYTHONPATH.  Nothing else of the package exists here."""
