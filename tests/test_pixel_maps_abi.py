"""CPU tests of the pixel-map entry points' boundary: the three symbols are exported and bound, and the
argument checks that need no device answer PMVS_EINVAL."""
import ctypes as C

import numpy as np

NAMES = ("pmvs_pixel_map_layout", "pmvs_loop_pixel_maps", "pmvs_pixel_maps_patches")


def test_pixel_map_symbols_exported(product_lib):
    import pmvs_amd as P
    for name in NAMES:
        assert name in P.EXPORTS
        fn = getattr(product_lib, name)  # AttributeError when the library does not export it
        assert fn.restype is C.c_int and fn.argtypes[-1] in (C.c_void_p, C.POINTER(P.DepthMapBuffers))
    for name in ("pixel_map_layout", "loop_pixel_maps", "pixel_maps_patches"):
        assert callable(getattr(P.Scene, name))


def test_pixel_maps_reject_null_arguments(product_lib):
    lib = product_lib
    import pmvs_amd as P
    buf = P.DepthMapBuffers()
    dims, off = np.zeros(2, np.int32), np.zeros(2, np.int64)
    assert lib.pmvs_pixel_map_layout(None, 0, 1, dims.ctypes.data, off.ctypes.data) == 1
    assert lib.pmvs_loop_pixel_maps(None, 0, 0, 1, 2, C.byref(buf)) == 1
    assert lib.pmvs_pixel_maps_patches(None, None, 0, 0, 0, 1, 2, C.byref(buf)) == 1
    assert lib.pmvs_last_error()
    # null buffers: a scene handle that is not null is not looked at before the check fails
    fake = C.c_void_p(1)
    assert lib.pmvs_loop_pixel_maps(fake, 0, 0, 1, 2, None) == 1
    assert lib.pmvs_pixel_maps_patches(fake, None, 0, 0, 0, 1, 2, None) == 1
