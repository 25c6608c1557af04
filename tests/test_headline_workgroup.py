"""The workgroups of variants 2 and 6 as the host sizes them (no GPU needed): fifteen waves on one staged copy of the scene
tables, an accumulator and a slab of 64 prepared rays per wave, two workgroups per CU -- and with the largest tables the
packer keeps LDS-resident, what a CU's workgroups need stays within its 160 KB of LDS.  Every other variant keeps the
4-wave workgroup, seven per CU."""
import pytest

CU_LDS = 160 * 1024
SIMD_WAVE_SLOTS = 8


@pytest.mark.parametrize("variant", [2, 6])
def test_big_groups_fit_a_cu_at_the_largest_resident_tables(rtmi, variant):
    g = rtmi.variant_workgroup(variant)
    waves = g["threads"] // 64
    assert g["threads"] == 15 * 64 and g["groups_per_cu"] == 2
    assert g["wave_lds"] == 192 * 8 + 64 * 10 * 4  # 64 pixels x rgb x 64 bits, 64 slots x {o, d, generator state}
    assert g["max_lds_bytes"] == g["max_table_bytes"] + waves * g["wave_lds"]
    assert g["groups_per_cu"] * g["max_lds_bytes"] <= CU_LDS, g
    # a workgroup's waves are dealt to the four SIMDs from the first one on: SIMD 0 holds ceil(waves / 4) of each group
    assert g["groups_per_cu"] * -(-waves // 4) <= SIMD_WAVE_SLOTS


@pytest.mark.parametrize("variant", [16, 36, 44, 52])
def test_other_variants_keep_four_waves(rtmi, variant):
    g = rtmi.variant_workgroup(variant)
    assert g["threads"] == 256 and g["wave_lds"] == 192 * 8 and g["groups_per_cu"] == 7
    assert g["groups_per_cu"] * g["max_lds_bytes"] <= CU_LDS, g


def test_unknown_variant_is_refused(rtmi):
    with pytest.raises(rtmi.RtmiError):
        rtmi.variant_workgroup(3)
    with pytest.raises(rtmi.RtmiError):
        rtmi.variant_workgroup(0)
