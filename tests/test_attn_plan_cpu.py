"""The KV split of the four-wave attention launch (kernels.h attn_plan), asked without a device through the diagnostics export s2v_diag_attn_plan.

attn_plan decides which trailing q-blocks of a head are cut by key range, into how many parts and where the parts begin.  The bitwise tests of the
suite (B = 1 == half of B = 2, head shards, per-item == persistent launch) rest on the rule seeing the token count and the attention format and
nothing else, so the export has exactly those two inputs.  Formats: 0 attn_q4, 1 attn_q4h, 2 attn_q4hh, 3 attn_q4f, 4 attn_q4fh (ATTN_FMT_*);
the fp8-QK^T formats 3 and 4 do not split."""
import ctypes
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {"q4": 0, "q4h": 1, "q4hh": 2, "q4f": 3, "q4fh": 4}
SPLITTING = ("q4", "q4h", "q4hh")
PARTS_MAX = 4        # ATTN_KV_PARTS
PP_MAX_TOKENS = 4608  # ATTN_PP_MAX_TOKENS: up to here attn_pp runs and nothing is split
LENGTHS = [4609, 4700, 4864, 5000, 19126, 50626]


def _pkg(name=""):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("disentangled-subject-to-vid_amd" + name)


@pytest.fixture(scope="module")
def diag():
    L = _pkg()._lib.diag_lib()
    L.s2v_diag_attn_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    return L


def plan(L, ntok, fmt):
    """(whole q-blocks per head, split q-blocks per head, S, shortest part allowed, [t_0 .. t_S])"""
    out = (ctypes.c_int32 * (4 + PARTS_MAX + 1))()
    assert L.s2v_diag_attn_plan(ntok, FORMATS[fmt], out) == 0, L.s2v_last_error()
    whole, split, S, tmin = out[0], out[1], out[2], out[3]
    t = list(out[4:4 + S + 1])
    assert all(x == -1 for x in out[4 + S + 1:]), "entries past t[S] are unused"
    return whole, split, S, tmin, t


@pytest.mark.parametrize("fmt", SPLITTING)
@pytest.mark.parametrize("ntok", LENGTHS)
def test_parts_tile_the_sequence(diag, ntok, fmt):
    whole, split, S, tmin, t = plan(diag, ntok, fmt)
    nqb, nt = (ntok + 255) // 256, (ntok + 63) // 64
    assert split >= 1 and whole + split == nqb
    assert 2 <= S <= PARTS_MAX
    assert t[0] == 0 and t[S] == nt, "the parts cover [0, nt)"
    lens = [t[s + 1] - t[s] for s in range(S)]
    assert all(n > 0 for n in lens), "contiguous and disjoint: the starts rise"
    assert max(lens) - min(lens) <= 1
    assert tmin >= 8 and min(lens) >= tmin, "no part shorter than what the body pre-stages, with margin"


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("ntok", [1, 64, 300, 511, 512, 1250, 4000, 4607, 4608])
def test_short_sequences_do_not_split(diag, ntok, fmt):
    """up to ATTN_PP_MAX_TOKENS the four-wave kernel runs only where the fp8 engine asks for its MX output: whole items.  The length rule (two parts
    of the shortest length need 2 x 8 tiles = 961 tokens) lies below that bound, so every length too short for two minimal parts is covered here."""
    whole, split, S, tmin, t = plan(diag, ntok, fmt)
    assert 2 * tmin * 64 <= PP_MAX_TOKENS
    assert (whole, split, S) == ((ntok + 255) // 256, 0, 1)
    assert t == [0, (ntok + 63) // 64]


@pytest.mark.parametrize("fmt", ["q4f", "q4fh"])
@pytest.mark.parametrize("ntok", LENGTHS)
def test_fp8_qk_formats_do_not_split(diag, ntok, fmt):
    whole, split, S, tmin, t = plan(diag, ntok, fmt)
    assert (whole, split, S) == ((ntok + 255) // 256, 0, 1) and t == [0, (ntok + 63) // 64]


def test_the_rule_sees_the_token_count_and_the_format_only(diag):
    """no argument through which a batch size, a head count or a CU count could enter, and the same answer on every call"""
    src = open(os.path.join(ROOT, "disentangled-subject-to-vid_amd", "csrc", "kernels.h")).read()
    assert "static inline AttnPlan attn_plan(int Ntok, int format) {" in src
    assert "void attn_plan_head(int Ntok, int format, int& whole, int& split, int& S) {" in src
    src = open(os.path.join(ROOT, "disentangled-subject-to-vid_amd", "csrc", "attention_q4.hip")).read()
    assert "int s2v_diag_attn_plan(int32_t Ntok, int32_t format, int32_t* out) {" in src
    assert plan(diag, 19126, "q4") == plan(diag, 19126, "q4")
    assert plan(diag, 19126, "q4")[:3] == plan(diag, 19126, "q4h")[:3] == plan(diag, 19126, "q4hh")[:3]


def test_flagship_item_list_is_pinned(diag):
    """49 x 480 x 720 with 226 text tokens: 19126 tokens = 75 q-blocks and 299 KV tiles per head.  73 whole q-blocks per head; the last full block
    and the ragged 182-row block in four parts each: B = 2, H = 48 launch 7008 whole items and 768 sub-items (7200 equal items before: 28.125
    rounds run as 29)"""
    whole, split, S, tmin, t = plan(diag, 19126, "q4")
    assert (whole, split, S) == (73, 2, 4)
    assert t == [0, 75, 150, 225, 299]
    B, H = 2, 48
    assert B * H * whole == 7008
    assert B * H * split * S == 768
    # the CFG-parallel half step
    assert 1 * H * whole == 3504 and 1 * H * split * S == 384
