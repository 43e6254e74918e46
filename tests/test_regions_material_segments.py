"""Material-temperature coupling on region slabs in segment mode, CPU side: the entry point
rt_material_enable_segments is declared in include/rtsn.h, exported by the built library and
bound by rtsn/api.py, and it checks its handle before anything touches a device.
"""
from __future__ import annotations

import ctypes as C


def test_enable_segments_declared_exported_and_null_checked(rtsn_mod):
    assert "rt_material_enable_segments" in rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    assert hasattr(L, "rt_material_enable_segments")
    fn = L.rt_material_enable_segments
    assert fn.argtypes == L.rt_material_enable_regions.argtypes  # the same arguments
    assert hasattr(rtsn_mod.Solver, "material_enable_segments")
    rho_cv = (C.c_double * 2)(1.0, 1.0)
    assert fn(None, rho_cv, 2, None) == 8  # RT_ERR_ARG: NULL handle
    assert b"rt_material_enable_segments" in L.rt_last_error(None)
