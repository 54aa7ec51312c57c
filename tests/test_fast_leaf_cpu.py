"""RL_FLAG_FAST_LEAF without a GPU: the definition's known answers (tests/fast_leaf_restatement.py) and the -fastleaf switch of the command line."""
import numpy as np
import pytest

import fast_leaf_restatement as FL
from ranklib_amd import _native as N
from ranklib_amd import evaluator
from ranklib_amd.learning import MART, LambdaMART, RankerType
from ranklib_amd._native import RankLibError


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_the_grouping_decides_a_known_answer():
    """2^53 followed by 256 ones.  Tile 0 = [2^53, 1 x 255]: step 128 gives a[0] = 2^53 + 1 -> 2^53 (the tie goes to the even mantissa) and 2 in the
    other entries; step 64: 2^53 + 2, entries of 4; then + 4, + 8, .., + 128: 2^53 + 254.  Tile 1 = [1] -> 1.  Level 1: (2^53 + 254) + 1 lies half way
    between 2^53 + 254 (odd mantissa) and 2^53 + 256 (even): 2^53 + 256.  A serial f64 sum never leaves 2^53."""
    x = np.concatenate([[2.0 ** 53], np.ones(256)])
    assert FL.B(x[:256]) == 2.0 ** 53 + 254
    assert FL.B(x[256:]) == 1.0
    assert FL.R(x) == 2.0 ** 53 + 256
    assert FL.serial_f64(x) == 2.0 ** 53
    # the order is part of the definition: with the ones first, tile 0 is 256 exactly and 2^53 + 256 needs no rounding at all
    assert FL.level(x[::-1])[0] == 256.0 and FL.R(x[::-1]) == 2.0 ** 53 + 256


def test_a_tile_is_folded_in_halves_not_left_to_right():
    # a[0] + a[128] meet first: 1 + 2^-53 is lost there, 2^-53 + 2^-53 on the other side is not
    x = np.zeros(256)
    x[0], x[128], x[1], x[129] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    assert FL.B(x) == 1.0 + 2.0 ** -52              # (1 + 2^-53 -> 1) + (2^-53 + 2^-53 = 2^-52)
    y = np.zeros(256)
    y[0], y[1], y[2], y[3] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    assert FL.B(y) == 1.0 + 2.0 ** -52              # step 2: a[0] + a[2] = 1 + 2^-53 -> 1 and a[1] + a[3] = 2^-52; step 1: a[0] + a[1]
    assert FL.serial_f64(y) == 1.0


def test_empty_single_and_signed_zero_segments():
    assert _bits(FL.R([])) == _bits(0.0)
    assert _bits(FL.R([3.25])) == _bits(3.25)       # one B: 3.25 + 0.0 eight times
    assert _bits(FL.R([-0.0])) == _bits(0.0)        # -0.0 + (+0.0) = +0.0 at the first step
    assert _bits(FL.R([-0.0] * 256)) == _bits(0.0)  # a full tile of -0.0 stays -0.0 through B; the final + 0.0 makes it +0.0
    assert _bits(FL.B([-0.0] * 256)) == _bits(-0.0)
    assert _bits(FL.R([-0.0] * 65536)) == _bits(0.0)
    assert _bits(FL.R([-0.0] * 257)) == _bits(0.0)


def test_levels():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(65537)
    l1 = FL.level(x)
    assert len(l1) == 257 and l1[256] == x[65536]
    l2 = FL.level(l1)
    assert len(l2) == 2 and l2[1] == x[65536]
    assert FL.R(x) == FL.B(l2)
    assert abs(FL.R(x) - FL.serial_f64(x)) < 1e-9


def test_output_rule():
    lam = np.array([0.5, -0.25, 2.0, 1.0])
    w = np.array([0.125, 0.25, 0.0, 0.0])
    assert FL.leaf_output(lam, w, [0, 1]) == np.float32(np.float32(0.25) / np.float32(0.375))
    assert FL.leaf_output(lam, w, [2, 3]) == np.float32(0)                      # s2 == 0 -> 0
    assert FL.leaf_output(lam, w, [0, 2, 3], mart=True) == np.float32(np.float32(3.5) / np.float32(3))


def test_flag_constant_and_abi_symbol():
    assert N.RL_FLAG_FAST_LEAF == 1
    assert N.RL_FLAG_FAST_LEAF & (N.RL_FLAG_TIMING | N.RL_FLAG_SERIAL_CHAIN | N.RL_FLAG_TIMING_NODES | N.RL_FLAG_JAVA_ORDER | N.RL_FLAG_FIRST_TIE) == 0
    assert "rl_debug_fast_sum" in N.ABI_SYMBOLS and callable(N.debug_fast_sum)


def test_rl_create_knows_the_flag_and_refuses_the_parity_modes_before_it_looks_for_a_device():
    for other in (N.RL_FLAG_JAVA_ORDER, N.RL_FLAG_SERIAL_CHAIN, N.RL_FLAG_JAVA_ORDER | N.RL_FLAG_FIRST_TIE):
        with pytest.raises(RankLibError) as e:
            N.Trainer(n_trees=1, flags=N.RL_FLAG_FAST_LEAF | other)
        assert "RL_FLAG_FAST_LEAF with RL_FLAG_" in str(e.value) and "(rlhip status -1)" in str(e.value)       # RL_ERR_INVALID
    with pytest.raises(RankLibError) as e:
        N.Trainer(n_trees=1, flags=64)
    assert "unknown bit in rl_params.flags" in str(e.value)
    try:        # the flag alone, and with RL_FLAG_FIRST_TIE (the speed-first pair), passes the argument checks: only a missing device can refuse it
        N.Trainer(n_trees=1, flags=N.RL_FLAG_FAST_LEAF).close()
        N.Trainer(n_trees=1, flags=N.RL_FLAG_FAST_LEAF | N.RL_FLAG_FIRST_TIE).close()
    except RankLibError as ex:
        assert "no CPU fallback" in str(ex) and "(rlhip status -5)" in str(ex)


def test_cli_sets_the_static_and_main_resets_it(monkeypatch):
    picked = []
    real = evaluator.Evaluator.__init__

    def spy(self, rtype, *a, **k):
        picked.append((rtype, LambdaMART.fastLeaf, MART.fastLeaf))
        real(self, rtype, *a, **k)
    monkeypatch.setattr(evaluator.Evaluator, "__init__", spy)
    assert LambdaMART.fastLeaf is False
    with pytest.raises(RankLibError):                      # the reader refuses the missing file after the flags are parsed
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "6", "-fastleaf"])
    assert picked[-1] == (RankerType.LAMBDAMART, True, True)          # MART inherits the static
    with pytest.raises(RankLibError):
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "0", "-FastLeaf"])        # flags are matched case-insensitively
    assert picked[-1] == (RankerType.MART, True, True)
    with pytest.raises(RankLibError):
        evaluator.main(["-train", "no_such_file.txt", "-ranker", "8"])
    assert picked[-1] == (RankerType.RANDOM_FOREST, False, False)    # main starts from False, like the other statics
    assert LambdaMART.fastLeaf is False
