"""The one-op references of tests/spk_ops_ref.py and tests/enc_unfold_ref.py pinned to what the project already trusts.  CPU only.

  * composed in spk_run's order (float64 convs over the unfolded rows) the speaker ops are tests/spk_ref.py's network, every stage
  * the clip unfold followed by a float64 one-tap matmul is tests/enc_ref.py's strided conv, in both padding modes
  * the streaming unfold (pushes plus carry) concatenates to the clip unfold bit for bit, for every split the GPU test runs
  * every real-data bound of the GPU test's cases stays under 2e-4 of the output's scale: a looser one-op bound would add nothing
  * the kernels' own order of sums, emulated in float32 numpy, is inside the bounds; a one-pass variance is not"""
import numpy as np
import pytest
import torch

from qwen3_tts_axera_russian_amd import weights as W
from tests import enc_ref
from tests import enc_unfold_ref as E
from tests import spk_common as C
from tests import spk_ops_ref as R
from tests import spk_ref


# ---- the speaker network from its one-op references -------------------------------------------------------------------
def compose(mel, state, sc):
    """spk_run's walk in float64 on one clip: every op through tests/spk_ops_ref.py, the convs as one-tap matmuls over the
    rows the unfold writes"""
    T = {k: np.asarray(v, np.float64) for k, v in state.items()}
    L = mel.shape[1]
    n_f = [L]

    def tdnn(p, x, c0, dil, x2=None, c02=0):
        w, b = T[p + ".conv.weight"], T[p + ".conv.bias"]
        cout, cin, k = w.shape
        rows = R.unfold(x, c0, cin, k, dil, n_f, x2, c02)[:, :, :L]
        raw = np.einsum("or,brl->bol", w.reshape(cout, cin * k), rows) + b[None, :, None]
        return R.place(raw, 0, cout, 1)

    out = {}
    cur = tdnn("blocks.0", mel[None], 0, sc.dilations[0])
    out["block0"] = cur[0]
    nb = len(sc.channels)
    Cw, cw = sc.channels[0], sc.channels[0] // sc.res2net_scale
    cat = np.zeros((1, sc.channels[-1], L))
    for i in range(1, nb - 1):
        h1 = tdnn(f"blocks.{i}.tdnn1", cur, 0, 1)
        r2 = np.zeros_like(h1)
        r2[:, :cw] = R.place(h1, 0, cw, 0)
        for j in range(1, sc.res2net_scale):
            r2[:, j * cw:(j + 1) * cw] = tdnn(f"blocks.{i}.res2net_block.blocks.{j - 1}", h1, j * cw, sc.dilations[i],
                                              r2 if j >= 2 else None, (j - 1) * cw)
        h2 = tdnn(f"blocks.{i}.tdnn2", r2, 0, 1)
        m, _ = R.rowmean(h2, n_f)
        hid, _ = R.matvec(T[f"blocks.{i}.se_block.conv1.weight"][:, :, 0], T[f"blocks.{i}.se_block.conv1.bias"], m, 1)
        gate, _ = R.matvec(T[f"blocks.{i}.se_block.conv2.weight"][:, :, 0], T[f"blocks.{i}.se_block.conv2.bias"], hid, 2)
        cur, _ = R.se_apply(h2, gate, cur)
        cat[:, (i - 1) * Cw:i * Cw] = cur
        out[f"block{i}"] = cur[0]
    xm = tdnn("mfa", cat, 0, sc.dilations[-1])
    out["mfa"] = xm[0]
    Cm = xm.shape[1]
    stat, _ = R.rowstat(xm, n_f)
    wt = T["asp.tdnn.conv.weight"][:, :, 0]
    abias, _ = R.matvec(wt[:, Cm:], T["asp.tdnn.conv.bias"], stat, 0)       # the mean / std columns as a per-clip bias
    raw = np.einsum("oc,bcl->bol", wt[:, :Cm], xm)
    att, _, _ = R.att_act(raw, abias)
    logit = np.einsum("oc,bcl->bol", T["asp.conv.weight"][:, :, 0], att) + T["asp.conv.bias"][None, :, None]
    pooled, _ = R.attnpool(logit, xm, n_f)
    out["asp"] = pooled[0]
    out["fc"] = R.matvec(T["fc.weight"][:, :, 0], T["fc.bias"], pooled, 0)[0][0]
    return out


def test_speaker_ops_compose_to_the_network():
    case = C.CASES["tiny"]
    sc, state = case["sc"], C.state("tiny")
    fb = W.spk_mel_filter_bank(sc)
    for n in case["lengths"]:
        mel = spk_ref.log_mel(C.seeded_clip(case["seed"], n), sc, fb)
        want, got = spk_ref.network(mel, state, sc), compose(mel, state, sc)
        assert set(C.STAGES) <= set(got)
        for s in C.STAGES:
            assert got[s].shape == want[s].shape, s
            err = float(np.abs(got[s] - want[s]).max())
            assert err <= 1e-12, f"{n} samples, stage {s}: {err:.2e}"


def test_unfold_is_exact_movement_and_one_add():
    """float32 in: the float32 add; columns past the clip +0; nothing of another clip's or the pad's columns"""
    x = R.rows((5, 9), 6, "real")
    x2 = R.rows((5, 9), 7, "real", 1)
    y = R.unfold(x, 1, 3, 3, 2, (5, 9), x2, 2)
    assert y.dtype == np.float32 and y.shape == (2, 9, 32) and np.isfinite(y).all()
    assert not y[0, :, 5:].any() and not y[1, :, 9:].any()
    want = np.pad(x[0, 1:4, :5], ((0, 0), (2, 2)), mode="reflect") + np.pad(x2[0, 2:5, :5], ((0, 0), (2, 2)), mode="reflect")
    for j in range(3):
        assert np.array_equal(y[0, j::3, :5], want[:, 2 * j:2 * j + 5])


# ---- the strided conv --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,replicate,elu", E.GEOMETRIES)
def test_clip_unfold_then_matmul_is_the_strided_conv(k, s, replicate, elu):
    r = np.random.default_rng([k, s, replicate, elu])
    cout = 3
    w = r.standard_normal((cout, 1, k))
    b = r.standard_normal(cout)
    flags = (W.EF_REPLICATE if replicate else 0) | (W.EF_ELU if elu else 0)
    tensors = {"enc.program": np.array([[W.EOP_CONV_S, 1, cout, k, s, flags, 0, 0]], np.int32), "enc.op0.weight": w, "enc.op0.bias": b}
    for n in E.CLIP_LENS(s):
        x = r.standard_normal(n).astype(np.float32)
        want, _ = enc_ref.enc_reference(tensors, x, dtype=torch.float64)
        v = E.clip_unfold(x[None, None, :], [n], k, s, replicate)[0]
        rows = E.elu64(v) if elu else v.astype(np.float64)
        got = w.reshape(cout, k) @ rows + b[:, None]
        assert got.shape == want.shape == (cout, -(-n // s))
        assert np.abs(got - want).max() <= 1e-12, (n, float(np.abs(got - want).max()))


def stream_through(x, k, s, replicate, pushes):
    """-> (the pushes' outputs side by side, [(live carry after the push or None)])"""
    st = E.StreamUnfold(x.shape[0], k, s, replicate)
    at, ys, carries = 0, [], []
    for n_in, fin in pushes:
        ys.append(st.push(x[:, at:at + n_in], fin))
        at += n_in
        carries.append(None if fin else st.carry[:, :st.cnt()].copy())
    assert at == x.shape[1]
    return np.concatenate(ys, axis=1), carries


@pytest.mark.parametrize("k,s,replicate,elu", E.GEOMETRIES)
def test_streaming_unfold_concatenates_to_the_clip_unfold(k, s, replicate, elu):
    r = np.random.default_rng([k, s, 77])
    for T in E.STREAM_T(s):
        x = r.standard_normal((3, T)).astype(np.float32)
        clip = E.clip_unfold(x[None], [T], k, s, replicate)[0]
        for name, pushes in E.splits(T, s, 5).items():
            assert sum(n for n, _ in pushes) == T and [f for _, f in pushes].count(1) == 1 and pushes[-1][1] == 1
            y, carries = stream_through(x, k, s, replicate, pushes)
            assert np.array_equal(y.view(np.uint32), clip.view(np.uint32)), f"T={T} split {name}"
            # the carry after a push is the tail of [padding | the stream so far]: the last (k - s) + total % s columns
            total = 0
            left = np.repeat(x[:, :1], k - s, axis=1) if replicate else np.zeros((3, k - s), np.float32)
            for (n_in, fin), c in zip(pushes, carries):
                total += n_in
                if fin:
                    continue
                if total == 0:
                    assert not c.any()          # nothing has come: the causal zeros, whatever the padding mode
                    continue
                seen = np.concatenate([left, x[:, :total]], axis=1)
                cnt = (k - s) + total % s
                assert np.array_equal(c.view(np.uint32), seen[:, seen.shape[1] - cnt:].view(np.uint32)), f"T={T} split {name}"
        if T % s:      # a finishing empty push behind a total that is no multiple of s: the last output comes out of the carry
            y, _ = stream_through(x, k, s, replicate, [(T, 0), (0, 1)])
            assert np.array_equal(y.view(np.uint32), clip.view(np.uint32))
    assert any(T % s for T in E.STREAM_T(s))


# ---- the bounds mean something ------------------------------------------------------------------------------------------
def capped(bound, ref, what, C=None):
    ratio = float((bound / (R.GRADE * R.scale_of(ref, C))).max())
    assert ratio <= 1.0, f"{what}: the bound is {ratio:.2f} of 2e-4 of the scale"
    return ratio


def test_every_real_data_bound_is_under_the_stage_grade():
    worst = {}
    note = lambda k, v: worst.__setitem__(k, max(v, worst.get(k, 0.0)))
    for lens in R.BATCHES:
        for Cc in R.CHANNELS:
            x = R.rows(lens, Cc, "real")
            ref, bound = R.rowmean(x, lens)
            note("rowmean", capped(bound, ref, f"rowmean {lens} C={Cc}"))
            ref, bound = R.rowstat(x, lens)
            note("rowstat", capped(bound, ref, f"rowstat {lens} C={Cc}", Cc))
            for kind in ("normal", "zero", "p80", "m1e4"):
                ref, bound = R.attnpool(R.attn_logits(lens, Cc, kind), x, lens)
                note("attnpool", capped(bound, ref, f"attnpool {kind} {lens} C={Cc}", Cc))
    for L in R.LENGTHS:
        x, names = R.rowstat_edge_rows(L)
        ref, bound = R.rowstat(x, [L])
        note("rowstat edge", capped(bound[:, [1, 2, 3, 5, 6, 7]], ref[:, [1, 2, 3, 5, 6, 7]], f"rowstat edge rows L={L}", 3))
        assert ref[0, 4] == np.sqrt(R.STD_FLOOR) and abs(ref[0, 0] - 0.25) < 1e-15           # the constant row is graded exactly instead
        se = R.se_case(L, 5, 3)
        ref, bound = R.se_apply(*se)
        note("se_apply", capped(bound, ref, f"se_apply L={L}"))
        ref, bound, zero = R.att_act(*R.att_case(L, 5, 3))
        note("att_act", capped(bound, ref, f"att_act L={L}"))
        assert 0.2 < zero.mean() < 0.35 and ref.max() > 0.999999
    for I in R.MATVEC_I:
        for O in R.CHANNELS:
            for with_bias in (False, True):
                w, bias, x = R.matvec_case(I, O, 3, with_bias)
                for act in (0, 1, 2):
                    ref, bound = R.matvec(w, bias, x, act)
                    note(f"matvec act {act}", capped(bound, ref, f"matvec I={I} O={O} bias={with_bias} act={act}"))
    print("worst bound / (2e-4 x scale):", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert R.TANH_ERR <= R.PROBE_CEILING and R.SIGMOID_ERR <= R.PROBE_CEILING
    assert R.TANH_MEASURED <= R.TANH_ERR and R.SIGMOID_MEASURED <= R.SIGMOID_ERR


# ---- the kernels' order of sums in float32 numpy -------------------------------------------------------------------------
def wave_sum32(lanes):
    v = np.asarray(lanes, np.float32).copy()
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[np.arange(64) ^ m]).astype(np.float32)
    return v[0]


def lanes32(terms, fma_scale=None):
    """lane-strided partial sums of a row of float32 terms; fma_scale: s = fma(m, term, s) (one rounding: through float64)"""
    s = np.zeros(64, np.float32)
    for l0 in range(0, len(terms), 64):
        t = np.asarray(terms[l0:l0 + 64])
        n = len(t)
        if fma_scale is None:
            s[:n] = s[:n] + t.astype(np.float32)
        else:      # float32 x float32 is exact in float64; the sum with s rounds once more, to float64 first: 29 spare bits
            s[:n] = (np.float64(fma_scale) * t.astype(np.float64) + s[:n].astype(np.float64)).astype(np.float32)
    return s


def rowstat32(x, one_pass=False):
    L = len(x)
    m = np.float32(1.0) / np.float32(L)
    mean = wave_sum32(lanes32(x, m))
    if one_pass:
        q = wave_sum32(lanes32((x * x).astype(np.float32), m)) - mean * mean
    else:
        d = (x - mean).astype(np.float32)
        q = wave_sum32(lanes32((d * d).astype(np.float32), m))
    return mean, np.sqrt(np.maximum(np.float32(q), np.float32(1e-12)), dtype=np.float32)


@pytest.mark.parametrize("L", [5, 6, 63, 64, 65, 129, 1000])
def test_emulated_kernel_order_is_inside_the_bounds(L):
    r = np.random.default_rng(L)
    worst = 0.0
    for mu, sd in ((0.0, 1.0), (4.0, 0.05), (-30.0, 2.0)):
        x = (mu + sd * r.standard_normal(L)).astype(np.float32)
        ref, bound = R.rowstat(x[None, None, :], [L])
        mean, std = rowstat32(x)
        err = np.abs(np.array([mean, std], np.float64) - ref[0])
        worst = max(worst, float((err / bound[0]).max()))
        assert (err <= bound[0]).all(), (L, mu, sd, err / bound[0])
        assert bound[0, 1] <= 1e-4 * ref[0, 1], "the std bound stays below 1e-4 of the std"
        if mu == 4.0:       # the mean is large against the spread: one pass loses the variance, and the bound notices
            _, std1 = rowstat32(x, one_pass=True)
            assert abs(float(std1) - ref[0, 1]) > bound[0, 1], (L, mu, sd)
        refm, boundm = R.rowmean(x[None, None, :], [L])
        got = np.float32(wave_sum32(lanes32(x)) / np.float32(L))
        assert abs(float(got) - refm[0, 0]) <= boundm[0, 0]
        short = np.float32(wave_sum32(lanes32(x[:64 * ((L - 1) // 64)] if L > 64 else x[:L - 1])) / np.float32(L))   # a dropped tail
        if mu:
            assert abs(float(short) - refm[0, 0]) > boundm[0, 0]
    print(f"L={L}: worst emulated error / bound {worst:.3f}")
