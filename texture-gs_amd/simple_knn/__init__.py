"""Drop-in for the `simple_knn` package of the 3D-GS lineage: `from simple_knn._C import distCUDA2` (models/gaussian3d.py:8)
resolves to the HIP implementation in texgs.points when texture-gs_amd/ is on PYTHONPATH."""
