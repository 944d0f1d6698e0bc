"""The refine layouts (PMVS_REFINE_CONFIG numbers, cmvs-pmvs_amd/csrc/pmvs_refine_layouts.h) that have a
bit-exact GPU case, and the (layout, wsize, tau) triples those cases run.  tests/test_refine_layouts.py
asserts that the layouts' union is exactly what the build instantiates, and that the triples reach every
kernel the launchers build: every layout at every wsize of its launcher's switch, and above tau = 8
wherever a kernel can hold more than 8 textures."""

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

SPLIT_CONFIGS = [c for c in REFINE_CONFIGS + NEW_CONFIGS if 200000 <= c < 300000]

# The wsize values each form's launcher instantiates its kernels for: the switches of launch_refine_lane
# (pmvs_refine_lane.hip), launch_refine (pmvs_kernels.hip, the wavefront form's launch_wave_ws) and
# launch_refine_split (pmvs_refine_split.hip).  A built kernel is (layout of the form, wsize of its set).
LANE_WSIZES = (5, 7, 9)
WAVE_WSIZES = (5, 7, 9)
SPLIT_WSIZES = (5, 7)

# (asked config, wsize, tau) of the GPU cases outside test_gpu_refine_envelope.py: the 8-view default
# scene (wsize 7, minImageNum 3: tau 6) of test_refine_configs_bit_exact and test_split_chain_configs_bit_exact,
# test_gpu_refine_fallbacks.py's two scenes, and the small (lane auto) batches of test_gpu_parity_matrix.py's
# wsize 5 and wsize 9 configurations.
DEFAULT_LARGE = 225019  # pmvs_api.cpp: the layout of the batches of small_n candidates or more
EXISTING_TRIPLES = [(c, 7, 6) for c in REFINE_CONFIGS + NEW_CONFIGS] + [
    (DEFAULT_LARGE, 9, 6),  # test_split_layout_at_wsize9_runs_wavefront_form
    (1206, 7, 14),          # test_wavefront_layout_below_tau_runs_2408
    (300000, 5, 6),         # test_refine_matrix[level0_w5_c1]
    (300000, 9, 4),         # test_refine_matrix[level2_w9_c4_min2]
]

# The envelope scenes of test_gpu_refine_envelope.py: conftest.small_scene(views, width, height, level=1,
# **kw); tau = min(2 * minImageNum, views) with minImageNum 3 unless given.  The smallest scenes on which
# the oracle still accepts about half of the synthetic candidates at these tau.
ENVELOPE_SCENES = {
    "w5_t6": dict(views=8, size=(480, 360), wsize=5, tau=6, kw=dict(wsize=5)),
    "w5_t14": dict(views=16, size=(320, 240), wsize=5, tau=14, kw=dict(arc_step_deg=6.0, wsize=5, min_image_num=7)),
    "w7_t9": dict(views=9, size=(320, 240), wsize=7, tau=9, kw=dict(arc_step_deg=8.0, min_image_num=5)),
    "w7_t16": dict(views=16, size=(320, 240), wsize=7, tau=16, kw=dict(arc_step_deg=6.0, min_image_num=8)),
    "w9_t14": dict(views=16, size=(480, 360), wsize=9, tau=14, kw=dict(arc_step_deg=6.0, wsize=9, min_image_num=7)),
}
ENVELOPE_SEED = 41  # synth_candidates' seed on every envelope scene

# (scene, asked config, batch size); "full" is CUs * G * CG + 777 candidates, every chain slot of a split
# layout's grid in use and refilled (test_gpu_split_chains._full).
ENVELOPE = (
    # wsize 5 at tau 6: all 13 split<5, *>, v2<5,12,6>, v2<5,24,8>, lane<5,4> and lane<5,8>
    [("w5_t6", c, 3000) for c in SPLIT_CONFIGS + [1206, 2408, 300004, 300008]]
    + [("w5_t6", c, 5) for c in (225019, 1206, 300004)]
    # tau 16: requests of 8-16 textures; 1206 runs 2408 on half the grid, 300000 and 300008 run 4 lanes per
    # texture (textures 9-16 on lanes 32-63), a 16-texture request fills an LP = 4 chunk exactly
    + [("w7_t16", c, 6000) for c in SPLIT_CONFIGS + [2408, 1206, 300000, 300004, 300008]]
    + [("w7_t16", c, "full") for c in (225019, 246014)]
    # tau 9: 1206 stays 1206 (12 slots, requests of up to 9 textures); the first tau at which 300000 takes 4
    + [("w7_t9", c, n) for c in (1206, 2408, 300000, 225019, 245016) for n in (6000, 5)]
    # wsize 5 above tau 8; 202032 is LP 1 (64 texture slots per chunk)
    + [("w5_t14", c, 6000) for c in (225019, 202032, 246014, 2408, 1206, 300000, 300008)]
    # wsize 9 above tau 8: the split layout falls back to 1206 and from there to v2<9,24,8>; lane<9,4> with
    # 21 samples x 3 channels per lane
    + [("w9_t14", c, n) for c in (225019, 2408, 300000) for n in (6000, 5)]
)
# The product's own choice on the scenes above tau 8: nothing set and a small batch (lane auto), and every
# batch on the default large layout (PMVS_REFINE_SMALL_N = 0).
ENVELOPE_DEFAULT_SMALL_N = 300
ENVELOPE_DEFAULT_LARGE_N = 6000
ENVELOPE_HIGH_TAU = [name for name, sc in ENVELOPE_SCENES.items() if sc["tau"] > 8]


def envelope_triples():
    """(asked config, wsize, tau) of every case of test_gpu_refine_envelope.py."""
    out = {(c, ENVELOPE_SCENES[name]["wsize"], ENVELOPE_SCENES[name]["tau"]) for name, c, _ in ENVELOPE}
    for name in ENVELOPE_HIGH_TAU:
        sc = ENVELOPE_SCENES[name]
        out.add((300000, sc["wsize"], sc["tau"]))
        out.add((DEFAULT_LARGE, sc["wsize"], sc["tau"]))
    return sorted(out)
