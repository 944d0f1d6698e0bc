/* tests/csrc/brick_layout.c -- prints sizeof/offsetof of the brick volume's structs in include/pmvs_amd.h so
 * tests/test_brick_abi.py can check the Python mirror's ctypes layouts against the C compiler. */
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"

#define S(T) printf("%s sizeof %zu\n", #T, sizeof(T))
#define O(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f))

int main(void) {
  S(pmvs_brick_params); O(pmvs_brick_params, tsdf); O(pmvs_brick_params, margin);
  S(pmvs_brick_buffers); O(pmvs_brick_buffers, brick); O(pmvs_brick_buffers, tsdf); O(pmvs_brick_buffers, obs);
  O(pmvs_brick_buffers, color);
  printf("PMVS_BRICK %d\nPMVS_BRICK_MAX_MARGIN %d\nPMVS_BRICK_MAX_DIM %d\n", PMVS_BRICK, PMVS_BRICK_MAX_MARGIN, PMVS_BRICK_MAX_DIM);
  return 0;
}
