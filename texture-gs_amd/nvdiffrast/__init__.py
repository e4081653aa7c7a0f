"""Drop-in for the one function of `nvdiffrast` that Texture-GS calls: `import nvdiffrast.torch as dr; dr.texture(...,
boundary_mode='cube')` (models/modules/NVDIFFREC/util.py:133, models/uv_map_gaussian3d.py:259) resolves to the HIP implementation
in texgs.cubetex when texture-gs_amd/ is on PYTHONPATH.  Nothing else of the package exists here."""
