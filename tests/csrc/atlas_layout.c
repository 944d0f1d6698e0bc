/* tests/csrc/atlas_layout.c -- prints sizeof/offsetof of the atlas's structs in include/pmvs_amd.h so
 * tests/test_atlas_abi.py can check the Python mirror's ctypes layouts against the C compiler. */
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"

#define S(T) printf("%s sizeof %zu\n", #T, sizeof(T))
#define O(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f))

int main(void) {
  S(pmvs_atlas_params); O(pmvs_atlas_params, width); O(pmvs_atlas_params, max_side); O(pmvs_atlas_params, scale);
  S(pmvs_atlas_layout); O(pmvs_atlas_layout, width); O(pmvs_atlas_layout, height); O(pmvs_atlas_layout, placed);
  O(pmvs_atlas_layout, cells);
  S(pmvs_atlas_buffers); O(pmvs_atlas_buffers, rgb); O(pmvs_atlas_buffers, texel_face); O(pmvs_atlas_buffers, uv);
  O(pmvs_atlas_buffers, atlas_view);
  printf("PMVS_ATLAS_MAX_SIDE value %d\n", PMVS_ATLAS_MAX_SIDE);
  printf("PMVS_ATLAS_MAX_WIDTH value %d\n", PMVS_ATLAS_MAX_WIDTH);
  return 0;
}
