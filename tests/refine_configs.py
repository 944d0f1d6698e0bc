"""The refine layouts (PMVS_REFINE_CONFIG numbers, cmvs-pmvs_amd/csrc/pmvs_refine_layouts.h) that have a
bit-exact GPU case.  tests/test_refine_layouts.py asserts that their union is exactly what the build
instantiates."""

# test_gpu_parity.py::test_refine_configs_bit_exact: lane form, wavefront form, split form
REFINE_CONFIGS = [300000, 300004, 300008, 1206, 2408, 202032, 224016, 225016, 226014, 227012, 228010, 245016, 246014,
                  248010]

# test_gpu_split_chains.py: the split layouts with 90-96 chains per CU
# 200000 + lanes per texture * 10000 + optimizer wavefronts * 1000 + chains per optimizer wavefront
NEW_CONFIGS = [226015, 226016, 225019, 227013]

# No layout: the retired workgroup form's number that round 5 ran for small batches and that older scripts
# still set.  test_refine_configs_bit_exact runs it too, for the rule "an unsupported PMVS_REFINE_CONFIG
# becomes 1206": the scene must give the oracle's records, not an error or another layout's launch.
RETIRED_CONFIG = 132042
