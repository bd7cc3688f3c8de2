"""A request's sampler-rules keys (batch_request.request_slot_rules, engine.SlotRules.check, batch_wire.pack_batch_request):
presets, overrides, every refusal, and the keys on a server without --sampler_rules.  No socket, no GPU."""
import json
import struct

import pytest

from qwen3_tts_axera_russian_amd.batch_request import RULE_KEYS, SAMPLER_PRESETS, request_has_rules, request_slot_rules
from qwen3_tts_axera_russian_amd.batch_wire import pack_batch_request
from qwen3_tts_axera_russian_amd.engine import SlotRules

UPSTREAM = SlotRules(rep_penalty=1.05, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=2)


def test_no_keys_no_rules():
    for msg in ({}, {"temperature": 0.5, "max_tokens": 9}, {k: None for k in RULE_KEYS}):
        assert not request_has_rules(msg)
        assert request_slot_rules(msg, True) is None and request_slot_rules(msg, False) is None


def test_presets():
    assert set(SAMPLER_PRESETS) == {"reference", "upstream"}
    assert request_slot_rules({"sampler": "reference"}, True) == SlotRules() and SlotRules().is_default()
    assert request_slot_rules({"sampler": "upstream"}, True) == UPSTREAM and not UPSTREAM.is_default()
    assert SlotRules() == SlotRules(rep_penalty=1.2, rep_window=30, eos_boost=15.0, eos_force=2.0, min_frames=0, cp_top_p=1.0)


def test_explicit_keys_override_the_preset():
    got = request_slot_rules({"sampler": "upstream", "repetition_penalty": 1.3, "min_tokens": 5, "cp_top_p": 0.8}, True)
    assert got == SlotRules(rep_penalty=1.3, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=5, cp_top_p=0.8)
    got = request_slot_rules({"repetition_window": 7, "eos_boost": 3, "eos_force": 1.5}, True)
    assert got == SlotRules(rep_window=7, eos_boost=3.0, eos_force=1.5)
    assert request_slot_rules({"repetition_window": 30.0, "min_tokens": 0.0}, True).is_default()      # integral floats, as top_k
    spelled = {"repetition_penalty": 1.2, "repetition_window": 30, "eos_boost": 15, "eos_force": 2, "min_tokens": 0, "cp_top_p": 1}
    assert request_slot_rules(spelled, True).is_default()


@pytest.mark.parametrize("msg", [
    {"sampler": "hf"}, {"sampler": 1}, {"sampler": ["upstream"]},
    {"repetition_penalty": 0.99}, {"repetition_penalty": "1.2"}, {"repetition_penalty": True}, {"repetition_penalty": float("nan")},
    {"repetition_penalty": float("inf")}, {"repetition_penalty": [1.2]},
    {"repetition_window": -1}, {"repetition_window": 31}, {"repetition_window": 2.5}, {"repetition_window": "3"}, {"repetition_window": False},
    {"eos_boost": -0.1}, {"eos_boost": float("inf")}, {"eos_boost": "15"},
    {"eos_force": -1}, {"eos_force": float("nan")}, {"eos_force": {}},
    {"min_tokens": -1}, {"min_tokens": 1.5}, {"min_tokens": 2 ** 31}, {"min_tokens": "2"},
    {"cp_top_p": 0}, {"cp_top_p": 1.01}, {"cp_top_p": -0.5}, {"cp_top_p": float("nan")}, {"cp_top_p": "1"},
    {"sampler": "upstream", "cp_top_p": 0},
    # values that are in range as doubles and out of it as the f32 the engine reads
    {"cp_top_p": 1e-50}, {"repetition_penalty": 1e39}, {"eos_boost": 1e39}, {"eos_force": 3.5e38}, {"eos_boost": 10 ** 400},
    {"repetition_penalty": 1 - 1e-9, "eos_boost": 1e39},
])
def test_refusals(msg):
    assert request_has_rules(msg)
    with pytest.raises(ValueError):
        request_slot_rules(msg, True)


@pytest.mark.parametrize("key,value", [("sampler", "reference"), ("sampler", "upstream"), ("repetition_penalty", 1.2),
                                       ("repetition_window", 30), ("eos_boost", 15), ("eos_force", 2), ("min_tokens", 0), ("cp_top_p", 1)])
def test_keys_without_the_flag_are_refused(key, value):
    with pytest.raises(ValueError):
        request_slot_rules({key: value}, False)               # even the default's values


def test_slot_rules_check():
    SlotRules().check()
    UPSTREAM.check()
    SlotRules(rep_penalty=1, rep_window=0, eos_boost=0, eos_force=0, min_frames=2 ** 31 - 1, cp_top_p=1e-6).check()
    for kw in (dict(rep_penalty=0.5), dict(rep_penalty=None), dict(rep_window=31), dict(rep_window=-1), dict(rep_window=3.0),
               dict(eos_boost=-1), dict(eos_force=float("inf")), dict(min_frames=-1), dict(min_frames=True), dict(cp_top_p=0),
               dict(cp_top_p=2), dict(cp_top_p="1")):
        with pytest.raises(ValueError):
            SlotRules(**kw).check()
    c = UPSTREAM.to_c()
    assert (c.rep_window, c.min_frames, list(c.reserved)) == (0, 2, [0, 0]) and abs(c.rep_penalty - 1.05) < 1e-6


def test_f32_rounding_keeps_what_is_in_range():
    assert request_slot_rules({"repetition_penalty": 1 - 1e-9}, True).rep_penalty == 1 - 1e-9     # 1.0f for the engine
    assert request_slot_rules({"cp_top_p": 1e-30, "eos_boost": 3e38}, True) == SlotRules(cp_top_p=1e-30, eos_boost=3e38)


def test_the_library_s_defaults_are_these_defaults():
    """q3e_default_rules (no GPU call) against engine.SlotRules and the test reference's table."""
    from qwen3_tts_axera_russian_amd import hiplib
    from tests import sample_rules_ref as RR
    lib = hiplib.load()
    c = hiplib.SlotRulesC(9.0, 9, 9.0, 9.0, 9, 9.0, (hiplib.ctypes.c_int32 * 2)(9, 9))
    lib.q3e_default_rules(hiplib.ctypes.byref(c))
    want = SlotRules().to_c()
    for name, _ in hiplib.SlotRulesC._fields_[:6]:
        assert getattr(c, name) == getattr(want, name), name
    assert list(c.reserved) == [0, 0]
    d = SlotRules()
    assert RR.DEFAULT == dict(rep_penalty=d.rep_penalty, rep_window=d.rep_window, eos_boost=d.eos_boost, eos_force=d.eos_force,
                              min_past=d.min_frames, cp_top_p=d.cp_top_p)
    lib.q3e_default_rules(None)                               # a null pointer is ignored


def test_the_client_sends_the_keys_only_when_given():
    def msg(**kw):
        raw = pack_batch_request(token_ids=[[1, 2]], **kw)
        (n,) = struct.unpack("<I", raw[:4])
        assert n == len(raw) - 4
        return json.loads(raw[4:])
    assert not request_has_rules(msg())
    m = msg(sampler="upstream", repetition_penalty=1.1, repetition_window=0, eos_boost=0.0, eos_force=0.0, min_tokens=3, cp_top_p=0.9)
    assert {k: m[k] for k in RULE_KEYS} == dict(sampler="upstream", repetition_penalty=1.1, repetition_window=0, eos_boost=0.0,
                                                 eos_force=0.0, min_tokens=3, cp_top_p=0.9)
    assert request_slot_rules(m, True) == SlotRules(rep_penalty=1.1, rep_window=0, eos_boost=0.0, eos_force=0.0, min_frames=3, cp_top_p=0.9)
