/* tests/csrc/fuse_layout.c -- prints sizeof/offsetof of the fusion's structs in include/pmvs_amd.h so
 * tests/test_fuse_abi.py can check the Python mirror's ctypes layouts against the C compiler. */
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"

#define S(T) printf("%s sizeof %zu\n", #T, sizeof(T))
#define O(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f))

int main(void) {
  S(pmvs_fuse_params); O(pmvs_fuse_params, radius); O(pmvs_fuse_params, min_support); O(pmvs_fuse_params, depth_rel);
  O(pmvs_fuse_params, normal_cos);
  S(pmvs_fuse_buffers); O(pmvs_fuse_buffers, support_map); O(pmvs_fuse_buffers, coord); O(pmvs_fuse_buffers, normal);
  O(pmvs_fuse_buffers, color); O(pmvs_fuse_buffers, support); O(pmvs_fuse_buffers, pixel); O(pmvs_fuse_buffers, patch);
  return 0;
}
