/* tests/csrc/texmesh_layout.c -- prints sizeof/offsetof of the texturing's structs in include/pmvs_amd.h so
 * tests/test_texmesh_abi.py can check the Python mirror's ctypes layouts against the C compiler. */
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"

#define S(T) printf("%s sizeof %zu\n", #T, sizeof(T))
#define O(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f))

int main(void) {
  S(pmvs_raster_buffers); O(pmvs_raster_buffers, face); O(pmvs_raster_buffers, depth);
  S(pmvs_texture_params); O(pmvs_texture_params, depth_rel); O(pmvs_texture_params, min_area);
  S(pmvs_texture_buffers); O(pmvs_texture_buffers, view); O(pmvs_texture_buffers, uv); O(pmvs_texture_buffers, score);
  return 0;
}
