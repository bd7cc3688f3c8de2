"""The encoder program against transformers' MimiModel.encode (tests/golden/mimi_encode_golden.npz, made by
tests/golden/make_mimi_encode_golden.py): the converter maps a MimiModel state dict, tests/enc_ref.py evaluates the
table, every stage and every code must match.  CPU only."""
import json
import os

import numpy as np
import pytest

from qwen3_tts_axera_russian_amd import weights as W
from tests import enc_common as C
from tests.enc_ref import enc_reference, rvq_encode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mimi_encode_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def case_state(gold, name):
    keys = json.loads(bytes(gold[f"{name}.keys"]).decode())
    state = C.seeded_state(C.CASES[name]["seed"], [(k, tuple(s)) for k, s in keys])
    assert C.digest(state) == bytes(gold[f"{name}.sha"]).decode(), "seeded tensors differ from the fixture's"
    return state


def case_table(gold, name):
    cfg = json.loads(bytes(gold[f"{name}.config"]).decode())
    return W.state_to_enc(case_state(gold, name), cfg, 16)


@pytest.mark.parametrize("name", list(C.CASES))
def test_converter_maps_every_key(gold, name):
    ec, t, report = case_table(gold, name)
    prog, shapes, _ = W.enc_program(ec)
    assert set(t) == set(shapes) | {"enc.program"}
    assert "decode-side" in report[0]
    # the decode half of the full MimiModel is in the state dict and was skipped, not consumed
    state = case_state(gold, name)
    assert any(k.startswith("decoder.") for k in state) and any(k.startswith("upsample.") for k in state)
    assert ec.n_q == 16 and len(np.asarray(t["enc.program"])) == len(prog)


@pytest.mark.parametrize("name", list(C.CASES))
def test_stray_key_is_an_error(gold, name):
    cfg = json.loads(bytes(gold[f"{name}.config"]).decode())
    state = case_state(gold, name)
    state["encoder.layers.1.block.5.conv.weight"] = np.zeros((4, 4, 1), np.float32)
    with pytest.raises(KeyError, match="no place in the table"):
        W.state_to_enc(state, cfg, 16)


def test_encoder_prefixed_dict_loads(gold):
    """A speech tokenizer nests the MimiModel under `encoder.` beside its own decoder (decoder.* of the tokenizer)."""
    cfg = json.loads(bytes(gold["mimi.config"]).decode())
    state = case_state(gold, "mimi")
    _, plain, _ = W.state_to_enc(state, cfg, 16)
    nested = {"encoder." + k: v for k, v in state.items()}
    nested["decoder.pre_conv.conv.weight"] = np.zeros((8, 8, 3), np.float32)   # the tokenizer's decoder: not ours
    _, t, _ = W.state_to_enc(nested, cfg, 16)
    assert set(t) == set(plain)
    for k in plain:
        np.testing.assert_array_equal(t[k], plain[k])


def test_speech_tokenizer_directory(gold, tmp_path):
    """convert_speech_tokenizer_encoder: safetensors under `encoder.` + config.json's encoder_config."""
    from safetensors.numpy import save_file
    cfg = json.loads(bytes(gold["mimi.config"]).decode())
    state = case_state(gold, "mimi")
    save_file({"encoder." + k: np.ascontiguousarray(v) for k, v in state.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({"encoder_config": cfg}))
    out = tmp_path / "enc.q3w"
    ec, report = W.convert_speech_tokenizer_encoder(str(tmp_path), str(out))
    assert any("encoder_valid_num_quantizers" in r for r in report)    # the default of 16 is said
    meta, t = W.read_pack(str(out))
    assert meta["enc_sample_rate"] == 24000
    _, plain, _ = W.state_to_enc(state, cfg, 16)
    for k in plain:
        np.testing.assert_array_equal(np.asarray(t[k]), plain[k])


@pytest.mark.parametrize("name", list(C.CASES))
def test_enc_ref_reproduces_every_stage_and_code(gold, name):
    case = C.CASES[name]
    ec, t, _ = case_table(gold, name)
    _, _, stages = W.enc_program(ec)
    stage_ops = dict(stages)
    n = case["lengths"][case["stage_clip"]]
    _, got = enc_reference(t, C.seeded_clip(case["seed"], n), len(W.enc_program(ec)[0]) - 1, stages=stage_ops)
    for st in stage_ops:
        ref = gold[f"{name}.{st}"]
        a = got[st][:, gold[f"{name}.{st}.cols"]]
        scale = float(np.abs(ref).max())
        err = float(np.abs(a - ref).max()) / max(scale, 1e-3)
        assert err <= 1e-5, f"{name} stage {st}: relative error {err:.2e}"
    for n in case["lengths"]:
        clip = C.seeded_clip(case["seed"], n)
        emb, _ = enc_reference(t, clip, stage_ops["embedding"])
        ref_emb = gold[f"{name}.embedding{n}"]
        assert np.abs(emb - ref_emb).max() <= 1e-5 * max(1.0, float(np.abs(ref_emb).max()))
        codes, _ = enc_reference(t, clip)
        want = gold[f"{name}.codes{n}"]
        assert codes.shape == want.shape == (W.enc_frames(ec, n), 16)
        assert (codes == want).all(), f"{name} n={n}: {(codes != want).sum()} ids differ"


def test_float64_grading_agrees_with_fixture(gold):
    """rvq_encode in float64 from the stored embedding gives the stored ids, and grading them gives ratio 1."""
    name = "other"
    ec, t, _ = case_table(gold, name)
    prog = np.asarray(t["enc.program"])
    proj = np.asarray(t[f"enc.op{len(prog) - 2}.weight"], np.float64)[:, :, 0]
    for n in C.CASES[name]["lengths"]:
        z = proj @ gold[f"{name}.embedding{n}"].astype(np.float64)
        codes, gap, ratio = rvq_encode(z, np.asarray(t[f"enc.op{len(prog) - 1}.codebook"], np.float64), 1,
                                       forced=gold[f"{name}.codes{n}"])
        assert (codes == gold[f"{name}.codes{n}"]).all()
        assert np.allclose(ratio, 1.0)
        np.testing.assert_allclose(gap, gold[f"{name}.gap{n}"], rtol=1e-9, atol=1e-12)


def test_frame_count_is_get_encoded_length():
    import torch
    from transformers import MimiConfig, MimiModel
    for name, case in C.CASES.items():
        cfg = MimiConfig(**case["cfg"])
        m = MimiModel(cfg)
        ec = W.enc_config_from_mimi(cfg.to_dict(), 16)
        hop = W.enc_hop(ec)
        for n in sorted({1, 2, hop - 1, hop, hop + 1, 2 * hop - 1, 2 * hop + 1, 3 * hop // 2, 7 * hop + 5, 24000, 240001}):
            assert W.enc_frames(ec, n) == int(m.get_encoded_length(torch.tensor(n))) == -(-n // hop), (name, n)
    assert W.enc_hop(W.EncConfig()) == 1920 and W.enc_frames(W.EncConfig(), 240000) == 125
