"""The decode-attention launch policy as a pure function of the module constants (no kernel library needed):
ops/native.decode_flags builds the `flags` word of ragk_attn_decode at call time, and shares the
single-partition decision with decode_partitions."""
import pytest

from rag_llm_k8s_amd.ops import native

NT, SINGLE, KL, DEFER = 1, 2, 4, 8  # attention.hip DEC_*; the DIAG value sits in bits 4-5


@pytest.fixture
def defaults(monkeypatch):
    monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 64)
    monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 256)
    monkeypatch.setattr(native, "DECODE_KL", True)
    monkeypatch.setattr(native, "DECODE_DIAG", 0)
    return monkeypatch


def test_flag_bits_match_the_kernel_source():
    assert (native.DEC_NT, native.DEC_SINGLE, native.DEC_KL, native.DEC_DEFER_MERGE) == (NT, SINGLE, KL, DEFER)
    assert native.DEC_DIAG_SHIFT == 4
    import os
    import re

    src = os.path.join(os.path.dirname(__file__), "..", "csrc", "kernels", "attention.hip")
    text = open(src).read()
    for name, bit in (("DEC_NT", 0), ("DEC_SINGLE", 1), ("DEC_KL", 2), ("DEC_DEFER_MERGE", 3)):
        assert re.search(r"\b%s = 1u << %d," % (name, bit), text), name
    assert re.search(r"\bDEC_DIAG_SHIFT = 4,", text)


@pytest.mark.parametrize("B,Hkv,want", [(63, 1, KL), (64, 1, NT | KL), (8, 8, NT | KL), (255, 1, NT | KL),
                                        (256, 1, NT | SINGLE | KL), (32, 8, NT | SINGLE | KL)])
def test_default_thresholds(defaults, B, Hkv, want):
    assert native.decode_flags(B, Hkv) == want
    assert native.decode_flags(B, Hkv, defer_merge=True) == want | DEFER
    assert native.decode_flags(B, Hkv, defer_merge=False) == want


def test_single_partition_grid_off(defaults):
    defaults.setattr(native, "DECODE_NW8_MIN_PAIRS", 0)
    assert native.decode_flags(32, 8) == NT | KL
    assert native.decode_flags(4096, 8) == NT | KL
    assert native.decode_partitions(8192, 32, 8) == (4, 2)  # ceil(512 / 256) partitions, not the single grid


def test_kl_on_off(defaults):
    defaults.setattr(native, "DECODE_KL", False)
    assert native.decode_flags(32, 8) == NT | SINGLE
    assert native.decode_flags(1, 8) == 0
    defaults.setattr(native, "DECODE_KL", True)
    assert native.decode_flags(32, 8) == NT | SINGLE | KL
    assert native.decode_flags(1, 8) == KL


@pytest.mark.parametrize("diag", [0, 1, 2])
def test_diag_bits(defaults, diag):
    defaults.setattr(native, "DECODE_DIAG", diag)
    assert native.decode_flags(32, 8) == NT | SINGLE | KL | (diag << 4)
    assert native.decode_flags(1, 1, defer_merge=True) == KL | DEFER | (diag << 4)


def test_constants_are_read_at_call_time(defaults):
    assert native.decode_flags(8, 8) == NT | KL
    defaults.setattr(native, "DECODE_NT_MIN_BH", 65)
    assert native.decode_flags(8, 8) == KL
    defaults.setattr(native, "DECODE_NW8_MIN_PAIRS", 64)
    assert native.decode_flags(8, 8) == SINGLE | KL


@pytest.mark.parametrize("min_pairs", [0, 1, 64, 256])
@pytest.mark.parametrize("B,Hkv", [(1, 1), (1, 8), (8, 8), (32, 8), (63, 1), (64, 1), (255, 1), (256, 1)])
@pytest.mark.parametrize("max_kv_len", [1, 256, 257, 8192])
def test_single_flag_is_the_pair_threshold_of_decode_partitions(defaults, min_pairs, B, Hkv, max_kv_len):
    """SINGLE is set exactly when decode_partitions returns max_parts == 1 BECAUSE of the pair threshold: a short
    context that also gets one partition below the threshold keeps the 4-wave split-K kernel."""
    defaults.setattr(native, "DECODE_NW8_MIN_PAIRS", min_pairs)
    single = bool(native.decode_flags(B, Hkv) & SINGLE)
    assert single == (min_pairs > 0 and B * Hkv >= min_pairs)
    _, mp = native.decode_partitions(max_kv_len, B, Hkv)
    if single:
        assert mp == 1
    # without the threshold the split follows the context length alone
    defaults.setattr(native, "DECODE_NW8_MIN_PAIRS", 0)
    _, mp_split = native.decode_partitions(max_kv_len, B, Hkv)
    assert not native.decode_flags(B, Hkv) & SINGLE
    if not single:
        assert mp == mp_split


def test_short_context_below_the_threshold_is_not_single(defaults):
    assert native.decode_partitions(200, 2, 2) == (4, 1)  # 4 tiles, at least 4 per partition
    assert native.decode_flags(2, 2) == KL
