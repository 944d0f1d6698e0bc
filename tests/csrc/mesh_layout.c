/* tests/csrc/mesh_layout.c -- prints sizeof/offsetof of the meshing's structs in include/pmvs_amd.h so
 * tests/test_mesh_abi.py can check the Python mirror's ctypes layouts against the C compiler. */
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"

#define S(T) printf("%s sizeof %zu\n", #T, sizeof(T))
#define O(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f))

int main(void) {
  S(pmvs_volume); O(pmvs_volume, origin); O(pmvs_volume, voxel); O(pmvs_volume, dims);
  S(pmvs_tsdf_params); O(pmvs_tsdf_params, fuse); O(pmvs_tsdf_params, trunc);
  S(pmvs_tsdf_buffers); O(pmvs_tsdf_buffers, tsdf); O(pmvs_tsdf_buffers, obs); O(pmvs_tsdf_buffers, color);
  S(pmvs_mesh_buffers); O(pmvs_mesh_buffers, vertex); O(pmvs_mesh_buffers, normal); O(pmvs_mesh_buffers, color);
  O(pmvs_mesh_buffers, face);
  return 0;
}
