"""Every session option in ONE pool and one sequence of steps, so that the hand-offs between the phases of a push -- intake,
quantiser, fork, WaveNet, emit and cross-fade, tail flush, resample, wire convert; place, resample, STFT, WaveNet, quantiser -- are
exercised together and not only option by option.  Every comparison is torch.equal.  The reference of a slot is the same session fed
the same pushes ALONE in a one-slot pool built with the same options: the path the neighbouring files hold to decode() / encode()
and to the host references of utils/.  The exact f32 slots are also held to decode() / encode() of their whole clip directly.

The launches of the whole script are counted once: convert, fork and cross-fade through the library's profile counters, the
resample launches at the C entry (the library keeps no record of its own for them).  Each count equals the number of steps that had
at least one member for that launch, worked out from the script with host schedules and from the lone runs' pieces."""
import random

import pytest
import torch

from dmel_codec_amd.models.stream_schedule import DecodeSchedule, EarlyDecodeSchedule, ResampleSchedule
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

F, UP, RATE = 4, 256, 24000                            # mel frames per token, samples per frame, the codec's and the vocoder's rate


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


class Launches:
    """the launches of the block: {"pcm_convert", "stream_fork", "crossfade"} from the profile counters, "resample" at the C entry"""

    def __enter__(self):
        from dmel_codec_amd import _lib
        self._lib, self.lib = _lib, _lib.lib()
        self.entry, self.count = self.lib.dmel_resample_window_items_f32, {"resample": 0}

        def counted(*args):
            self.count["resample"] += 1
            return self.entry(*args)
        self.lib.dmel_resample_window_items_f32 = counted
        _lib.prof_reset(); _lib.prof_enable(True)
        return self

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize()
            for family in ("pcm_convert", "stream_fork", "crossfade"):
                self.count[family] = self._lib.prof_read(family)["launches"]
        finally:
            self._lib.prof_enable(False); self._lib.prof_reset()
            self.lib.dmel_resample_window_items_f32 = self.entry


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ decode
DEC_POOL = dict(max_push_tokens=8, early_emit=True, crossfade_samples=UP, output_sample_rates=(48000, 8000))
DEC_OPEN = [dict(),                                                                                   # exact, f32, mono
            dict(lookahead_frames=0, crossfade_samples=UP, output_sample_rate=48000, sample_format="s16", channels=2),
            dict(lookahead_frames=8, output_sample_rate=8000, sample_format="ulaw"),
            dict(lookahead_frames=4, crossfade_samples=UP),                                          # vocoder rate, f32
            dict(output_sample_rate=48000)]                                                           # exact, f32
DEC_ENDS, DEC_LAST = {1: 17, 3: 22}, 29                # slot 1 ends WITHOUT tokens, slot 3 with some; the others with the script
DEC_MOVES = {12: (2, 2)}                               # in front of step 12: set_lookahead(slot 2, 2)


def decode_script():
    """[({slot: tokens}, the slots that end)] per step, seeded: 0 .. 8 tokens, every slot idle in about one step of five"""
    rng, steps = random.Random(2024), []
    for t in range(DEC_LAST + 1):
        plan, final = {}, []
        for s in range(len(DEC_OPEN)):
            end = DEC_ENDS.get(s, DEC_LAST)
            if t == end:
                plan[s] = 0 if s == 1 else rng.randint(1, 8)
                final.append(s)
            elif t < end and rng.random() < 0.8:
                plan[s] = rng.choice([0, 1, rng.randint(0, 8), 8, 8])
        steps.append((plan, tuple(final)))
    return steps


def decode_run(codec, dev, script, clips, only=None):
    """the script on a pool of all sessions (only=None) or of session `only` alone -> ({session: [(audio, mel) per push]}, origins)"""
    members = list(range(len(DEC_OPEN))) if only is None else [only]
    pool = codec.decode_sessions(len(members), **DEC_POOL)
    slot = {i: pool.open(**DEC_OPEN[i]) for i in members}
    pos, got, origins = {i: 0 for i in members}, {i: [] for i in members}, []
    for t, (plan, final) in enumerate(script):
        if t in DEC_MOVES and DEC_MOVES[t][0] in slot:
            pool.set_lookahead(slot[DEC_MOVES[t][0]], DEC_MOVES[t][1])
        plan = {i: n for i, n in plan.items() if i in slot}
        if not plan:
            continue
        ids, noise = {}, {}
        for i, n in plan.items():
            a = pos[i]
            pos[i] += n
            ids[slot[i]], noise[slot[i]] = clips[i][0][:, a:a + n], clips[i][1][:, F * a:F * (a + n)]
        out = pool.push(ids, noise=noise, final=[slot[i] for i in final if i in slot])
        assert set(out) == set(ids)
        for i in plan:
            got[i].append(out[slot[i]])
        origins.append(max(pool.origin))
    assert pool.open_slots == []
    return got, origins


def decode_members(geo, script, ref):
    """the steps of the script with at least one member for the fork, the cross-fade, the resample and the convert launch"""
    mirror = [EarlyDecodeSchedule(geo, o["lookahead_frames"], fade_frames=1 if o.get("crossfade_samples") else 0)
              if "lookahead_frames" in o else DecodeSchedule(geo) for o in DEC_OPEN]
    has_tail, at = [False] * len(DEC_OPEN), [0] * len(DEC_OPEN)
    count = dict(stream_fork=0, crossfade=0, resample=0, pcm_convert=0)
    for t, (plan, final) in enumerate(script):
        if t in DEC_MOVES:
            mirror[DEC_MOVES[t][0]].set_lookahead(DEC_MOVES[t][1])
        member = dict.fromkeys(count, False)
        for i, n in plan.items():
            st, o = mirror[i].step(n, i in final), DEC_OPEN[i]
            audio = ref[i][at[i]][0]
            at[i] += 1
            member["stream_fork"] |= "lookahead_frames" in o and st.shadow
            if o.get("crossfade_samples") and st.voc_window[1] > st.voc_window[0]:
                member["crossfade"] |= has_tail[i] or i not in final               # a tail to blend with, or a new one to save
                has_tail[i] = i not in final
            member["resample"] |= "output_sample_rate" in o and audio.numel() > 0
            member["pcm_convert"] |= (o.get("sample_format", "f32") != "f32" or o.get("channels", 1) > 1) and audio.numel() > 0
        for k, v in member.items():
            count[k] += bool(v)
    return count


def test_decode_pool_with_every_option_returns_what_each_session_returns_alone(dev, codec):
    """5 slots: exact f32 | k = 0, fade of a frame, 48 kHz, s16, stereo | k = 8 then 2, 8 kHz, mu-law | k = 4, fade, vocoder rate |
    exact at 48 kHz.  30 steps of 0 .. 8 tokens, subsets of the slots, explicit noise.  Slot 1 ends with a push of 0 tokens: a fading
    slot that ends without new frames, at another rate, through the wire convert.  The slots are re-based on the way (cap = 288
    frames, more than 72 tokens per slot)."""
    script = decode_script()
    assert any(len(plan) < len(DEC_OPEN) and t < min(DEC_ENDS.values()) for t, (plan, _) in enumerate(script))
    total = [sum(plan.get(i, 0) for plan, _ in script) for i in range(len(DEC_OPEN))]
    g = torch.Generator().manual_seed(31)
    clips = [(torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev),
              torch.randn(codec.decoder.residual_channels, T * F, generator=g).to(dev)) for T in total]
    with Launches() as seen:
        got, origins = decode_run(codec, dev, script, clips)
    assert max(origins) > 0, "no slot was re-based"
    ref = {}
    for i in range(len(DEC_OPEN)):
        ref.update(decode_run(codec, dev, script, clips, only=i)[0])
    for i in range(len(DEC_OPEN)):
        assert len(got[i]) == len(ref[i]) > 0
        for j, ((a, m), (ra, rm)) in enumerate(zip(got[i], ref[i])):
            assert same(m, rm), f"session {i}, push {j}: mel"
            assert same(a, ra), f"session {i}, push {j}: audio"
    # the wire of every slot, and the corner: slot 1's last piece is its held-back tail alone, resampled and converted
    assert got[1][-1][1].shape[1] == 0 and got[1][-1][0].dtype == torch.int16 and got[1][-1][0].shape[1] == 2
    assert got[1][-1][0].shape[0] > 0
    assert got[2][-1][0].dtype == torch.uint8 and got[3][-1][1].shape[1] > 0
    # the exact f32 slot against decode() of its ids
    ids, noise = clips[0]
    audio, mel = codec.decode(ids[None].contiguous(), torch.tensor([total[0]], device=dev), return_audios=True, noise=noise[None].contiguous())
    assert torch.equal(torch.cat([a for a, _ in got[0]], dim=1), audio[0]) and torch.equal(torch.cat([m for _, m in got[0]], dim=1), mel[0])
    want = decode_members(codec.decode_sessions(1, **DEC_POOL).geo, script, ref)
    assert min(want.values()) > 0
    assert seen.count == want


# ------------------------------------------------------------------------------------------------------------ encode
ENC_POOL = dict(max_push_samples=2048, sample_rates=(48000, 8000))
ENC_OPEN = [dict(),                                                                                   # f32 at the codec's rate
            dict(sample_rate=48000, sample_format="s16", channels=2),
            dict(sample_rate=8000, sample_format="alaw"),
            dict(sample_rate=48000, channels=2, channel=1)]                                           # f32, the right channel
ENC_ENDS, ENC_LAST, ENC_MONO = {2: 8, 1: 10}, 13, 5    # slot 2 ends WITHOUT samples, slot 1 with some; step 5 names slot 0 alone


def encode_script():
    """[({slot: samples of its own rate}, the slots that end)] per step, seeded: 0 .. 2048 samples; two full pushes first, so that
    every clip is longer than the reflect pad when it ends"""
    rng, steps = random.Random(23), []
    for t in range(ENC_LAST + 1):
        plan, final = {}, []
        for s in range(len(ENC_OPEN)):
            end = ENC_ENDS.get(s, ENC_LAST)
            if t == ENC_MONO:
                if s == 0:
                    plan[s] = rng.randint(1, 2048)
            elif t == end:
                plan[s] = 0 if s == 2 else rng.randint(1, 2048)
                final.append(s)
            elif t < 2:
                plan[s] = 2048
            elif t < end and rng.random() < 0.8:
                plan[s] = rng.choice([0, 1, rng.randint(0, 2048), 2048])
        steps.append((plan, tuple(final)))
    return steps


def encode_run(codec, script, clips, only=None):
    members = list(range(len(ENC_OPEN))) if only is None else [only]
    pool = codec.encode_sessions(len(members), **ENC_POOL)
    slot = {i: pool.open(**ENC_OPEN[i]) for i in members}
    pos, got = {i: 0 for i in members}, {i: [] for i in members}
    for plan, final in script:
        plan = {i: n for i, n in plan.items() if i in slot}
        if not plan:
            continue
        audio = {}
        for i, n in plan.items():
            audio[slot[i]] = clips[i][pos[i]:pos[i] + n]
            pos[i] += n
        out = pool.push(audio, final=[slot[i] for i in final if i in slot])
        assert set(out) == set(audio)
        for i in plan:
            got[i].append(out[slot[i]])
    assert pool.open_slots == []
    return got


def encode_members(script):
    mirror = [ResampleSchedule(o["sample_rate"], RATE) if "sample_rate" in o else None for o in ENC_OPEN]
    wired = [o.get("sample_format", "f32") != "f32" or o.get("channels", 1) > 1 for o in ENC_OPEN]
    count = dict(stream_fork=0, crossfade=0, resample=0, pcm_convert=0)
    for plan, final in script:
        released = [mirror[i].step(n, i in final).outputs for i, n in plan.items() if mirror[i] is not None]
        count["resample"] += any(b > a for a, b in released)
        count["pcm_convert"] += any(wired[i] for i in plan) and any(plan.values())
    return count


def test_encode_pool_with_every_option_returns_what_each_session_returns_alone(dev, codec):
    """4 slots: f32 at the codec's rate | 48 kHz, s16, stereo | 8 kHz, A-law | 48 kHz, f32, stereo, channel 1.  14 steps of
    0 .. 2048 samples of each slot's own rate, subsets of the slots, one step that names the mono f32 slot alone (the float path:
    no convert launch); slot 2 ends with an empty push on step 8, slot 1 with samples on step 10."""
    script = encode_script()
    assert set(script[ENC_MONO][0]) == {0} and any(len(plan) in (2, 3) for plan, _ in script[:min(ENC_ENDS.values())])
    total = [sum(plan.get(i, 0) for plan, _ in script) for i in range(len(ENC_OPEN))]
    g = torch.Generator().manual_seed(32)
    clips = [(torch.randn(total[0], generator=g) * 0.3).to(dev),
             (torch.randn(total[1], 2, generator=g) * 0.2 * 32768).round().clamp(-32768, 32767).to(torch.int16).to(dev),
             torch.randint(0, 256, (total[2],), generator=g, dtype=torch.uint8).to(dev),
             (torch.randn(total[3], 2, generator=g) * 0.3).to(dev)]
    with Launches() as seen:
        got = encode_run(codec, script, clips)
    for i in range(len(ENC_OPEN)):
        ref = encode_run(codec, script, clips, only=i)[i]
        assert len(got[i]) == len(ref) > 0 and sum(x.shape[1] for x in ref) > 0
        for j, (x, y) in enumerate(zip(got[i], ref)):
            assert same(x, y), f"session {i}, push {j}"
    ids, lens = codec.encode(clips[0][None], torch.tensor([total[0]], device=dev))
    assert torch.equal(torch.cat(got[0], dim=1), ids[0][:, :int(lens[0])])
    want = encode_members(script)
    assert want["resample"] > 0 and 0 < want["pcm_convert"] < sum(1 for plan, _ in script if any(plan.values()))
    assert seen.count == want
