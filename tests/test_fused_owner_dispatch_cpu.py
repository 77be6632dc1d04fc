"""ops.fused_dq_owner_mode: which form of the fused attention backward forms dq.  Owner mode runs B H equally long workgroups, one per
compute unit at a time; it is chosen when they fill the usable units without a long tail."""
from symbolic_music_generation_amd.ops import FUSED_OWNER_MIN_FILL, fused_dq_owner_mode


def test_whole_rounds_choose_owner_mode():
    assert fused_dq_owner_mode(64, 12, 256)          # 768 workgroups: three full rounds (the C3 training step)
    assert fused_dq_owner_mode(64, 8, 256)           # 512: two full rounds
    assert fused_dq_owner_mode(32, 8, 256)           # 256: one


def test_a_long_tail_stays_on_the_per_block_grid():
    assert not fused_dq_owner_mode(32, 12, 256)      # 384 workgroups: the second round is half empty (mode S, published base)
    assert not fused_dq_owner_mode(2, 2, 256)        # the small shapes of the test suite
    assert not fused_dq_owner_mode(16, 12, 256)      # 192 of 256


def test_the_rule_is_the_tail_efficiency_against_the_threshold():
    for wgs in range(1, 1100, 7):
        rounds = -(-wgs // 256)
        assert fused_dq_owner_mode(wgs, 1, 256) == (wgs / (rounds * 256) >= FUSED_OWNER_MIN_FILL), wgs


def test_reserved_units_shift_it():
    assert not fused_dq_owner_mode(64, 12, 256, reserved=16)     # 768 on 240 units: 3.2 rounds
    assert fused_dq_owner_mode(60, 12, 256, reserved=16)         # 720 on 240: three full rounds
    assert fused_dq_owner_mode(125, 4, 256) and not fused_dq_owner_mode(125, 4, 256, reserved=16)      # 500: 0.98 of 512, 0.69 of 720
    assert fused_dq_owner_mode(1, 8, 256, reserved=250)          # never fewer than 8 usable units


def test_the_environment_overrides_it():
    assert not fused_dq_owner_mode(64, 12, 256, env={'MXL_FUSED_OWNER': '0'})
    assert fused_dq_owner_mode(32, 12, 256, env={'MXL_FUSED_OWNER': '1'})
    assert fused_dq_owner_mode(64, 12, 256, env={'MXL_FUSED_OWNER': ''})
    assert not fused_dq_owner_mode(32, 12, 256, env={})
