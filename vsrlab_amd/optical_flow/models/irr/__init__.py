"""``vsrlab.optical_flow.models.irr``: of the reference's IRR-PWC only the cost volume (``pwc_modules.compute_cost_volume``), on
the HIP path (``csrc/spatial_corr.hip``).  Why the network itself is not here: DESIGN section 11f."""
