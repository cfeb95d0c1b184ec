"""Static audit of the compiled gfx950 code of the voting kernels (no GPU needed): the hand-written
wave loops name physical registers, so the kernels must not spill vector registers nor use scratch,
and must stay within 64 VGPRs (8 waves per SIMD = two 1024-thread workgroups per CU; 128 for the
vector-fill kernels, which run one workgroup per CU)."""
import re

import pytest

from kernel_asm import _hipcc, kernel_asm_text


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_vote_kernels_do_not_spill():
    text = kernel_asm_text()
    seen = 0
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_vote_" not in name:
            continue
        seen += 1
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        vector_fill = "k_vote_bands_vfill" in name or "k_vote_fuse_argmax" in name
        if "k_vote_fuse_argmax_2cu" in name:
            # the two-workgroups-per-CU variant of the fused kernel (bands of at most half the LDS): 64 VGPRs hold the
            # wave loops' ~30 named registers OR the per-cell state (10 + 10 + 3) plus the read-back's temporaries, so
            # the compiler parks part of the state in scratch AROUND the assembly blocks -- once per phase, never inside
            # a wave loop (the loops are single asm statements).  Bounded here so that it cannot grow unnoticed.
            assert val("vgpr_count") <= 64, name
            assert val("vgpr_spill_count") <= 32 and val("private_segment_fixed_size") <= 64, name
            continue
        if "k_vote_fuse_argmax" in name and "ELb1ELb0EE" in name:
            # the two-camera instantiation that parks camera 1's values in a second register array (round 6, DEFER): at the
            # 128-register limit of a 16-wave workgroup; a handful of values go to scratch AROUND the assembly blocks (once
            # per phase).  Bounded so that it cannot grow unnoticed.
            assert val("vgpr_count") <= 128, name
            assert val("vgpr_spill_count") <= 8 and val("private_segment_fixed_size") <= 32, name
            continue
        if vector_fill:
            # lane mappings 5 / 6 run where ONE workgroup fills a CU (wide grids): 4 waves per SIMD, up to
            # 128 VGPRs -- the third register set of gathers in flight lives there; the fused vote -> fusion
            # -> arg-max kernel keeps camera 0's values and the running maxima of <= 20 cells per thread in
            # registers across the wave loops (which name 32-40 registers themselves): no spill there either
            assert val("vgpr_count") <= 128, name
        else:
            # 8 waves per SIMD (two 1024-thread workgroups per CU) need <= 64 VGPRs -- the persistent loop
            # once pushed the all-in-one packed kernel to 70 and cost 15 % at 346x260x100
            assert val("vgpr_count") <= 64, name
        assert val("vgpr_spill_count") == 0 and val("private_segment_fixed_size") == 0, name
        # (scalar spills go to VGPR lanes with v_writelane / v_readlane outside the wave loops: harmless,
        #  the packed kernels hand ~15 scalars to each assembly block and keep ~30 for the item loop)
    assert seen >= 16
    # the resolver's kernels (round 5): no scratch either, but for the inverted event pass (below)
    tie = 0
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_tie_" not in name and "k_store_depth_map" not in name:
            continue
        tie += 1
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        if "k_tie_hits_binned" in name:
            # 512 threads at <= 64 VGPRs (8 waves per SIMD: four blocks per CU next to 4 x 38 KB of LDS); the compiler parks a
            # few values in scratch for that -- measured against 6 waves per SIMD without spills: 326 vs 419 us per camera
            assert val("vgpr_count") <= 64 and val("private_segment_fixed_size") <= 128, name
            continue
        assert val("vgpr_spill_count") == 0 and val("private_segment_fixed_size") == 0, name
        if "k_tie_sort_runs" in name or "k_tie_prove" in name:
            # a thread keeps up to 16 (key, bucket, rank, final slot) of its run in registers; the LDS (12 / 24 / 48 KB per
            # 256-thread workgroup), not the registers, bounds the occupancy of these kernels.  (k_tie_prove*: the proof's
            # per-column interval arithmetic in double precision, up to eight cameras' bounds at once -- a verification pass)
            assert val("vgpr_count") <= 128, name
            continue
        assert val("vgpr_count") <= 64, name
    assert tie >= 10
    # the hand-scheduled loops are in there and keep their waits
    assert text.count("s_waitcnt vmcnt(3)") >= 6 and "v_cvt_flr_i32_f32" in text and "v_cmpx_ge_u32" in text
