"""Live sessions that are parked, moved to another pool and branched (snapshot / drop / park / restore of EncodeSessions and
DecodeSessions) on the GPU.  Every comparison is torch.equal.  The reference of an encode session is encode() of its finished clip;
the reference of a decode session is the same script run uninterrupted in one pool, and decode() of its tokens for the exact ones.
A parked session's old rows are filled with NaN, its snapshot goes to the CPU, through torch.save / torch.load(weights_only=True) and
back, and is restored into a second pool of another slot count, maximal push and capacity whose free rows were filled with NaN too."""
import io

import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot
from dmel_codec_amd.models.stream_schedule import ResampleSchedule
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR, F = 24000, 4
MAX_PUSH = 16
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dec_codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


@pytest.fixture(scope="module")
def enc_codec(dev):
    return make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


# ------------------------------------------------------------------------------------------------------------ moving a session
def poison(pool, slots):
    """NaN (a wrong id for the tokens) in every row of device state the slots own, the shadow rows and the fade weights included"""
    if pool.buf is None:
        return
    b, G = pool.buf, pool.G
    for s in slots:
        if "feat" in b:                                                     # an encode pool
            b["mel"][s] = NAN
            b["samples"][s] = NAN
            for name in ("skip", "feat"):
                b[name][s * G:(s + 1) * G] = NAN
            b["hist"][:, s * G:(s + 1) * G] = NAN
        else:
            for row in (s, pool.S + s) if pool.early_emit else (s,):
                for name in ("skip", "cond", "mel"):
                    b[name][row] = NAN
                b["hist"][:, row] = NAN
            b["tokens"][s] = 3
            b["noise"][s] = NAN
            for name in ("fade_tail", "fade_w"):
                if name in b:
                    b[name][s] = NAN
        if pool.rs is not None and pool.rs.buf is not None:
            pool.rs.buf["rows"][s] = NAN


def through_a_file(snap, dev):
    assert snap.blob.is_cuda or snap.nbytes == 0
    host = snap.cpu()
    assert host.blob.device.type == "cpu" and host.nbytes == snap.nbytes and host.meta == snap.meta
    buf = io.BytesIO()
    torch.save(host.as_dict(), buf)
    assert buf.tell() < snap.nbytes + 16384                                 # its own words, not the launch's common blob
    buf.seek(0)
    back = SessionSnapshot.from_dict(torch.load(buf, weights_only=True))
    assert back.meta == snap.meta and torch.equal(back.blob, host.blob)
    return back.to(dev)


def move(pools, at, slot, dev):
    """park slot of pools[at], poison what it leaves, carry the snapshot through a file, restore into the other pool's poisoned rows"""
    src, dst = pools[at], pools[1 - at]
    snap = src.park([slot])[slot]
    assert slot not in src.open_slots
    poison(src, [slot])
    snap = through_a_file(snap, dev)
    poison(dst, [s for s in range(dst.S) if s not in dst.open_slots])
    [new] = dst.restore([snap])
    assert new in dst.open_slots
    return 1 - at, new, snap


# ------------------------------------------------------------------------------------------------------------ encode
# clip -> (format, rate, channels, seconds, push sizes in frames of its own rate, the pool it starts in, whether it moves)
ENC = {"f": ("f32", SR, 1, 3.7, [2048], 0, True),                          # long enough to be re-based (asserted)
       "s": ("s16", 48000, 2, 0.5, [300, 2048, 1, 2048], 0, True),
       "u": ("ulaw", 8000, 1, 0.6, [160, 2048, 0, 800], 0, True),
       "a": ("f32", SR, 1, 0.7, [2048, 0, 1500], 0, False),                # neighbours that are never named in park / restore
       "b": ("f32", SR, 1, 0.7, [1, 2048], 1, False)}
_enc = {}


def enc_clip(fmt, n, ch, seed, dev):
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if ch == 1 else (n, ch)
    x = torch.randn(shape, generator=g) * 0.2
    if fmt == "s16":
        x = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    elif fmt == "ulaw":
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return x.to(dev)


def encode_run(codec, dev):
    if _enc:
        return _enc
    from dmel_codec_amd.utils import pcm
    pools = [codec.encode_sessions(slots=4, max_push_samples=2048, sample_rates=(48000, 8000)),
             codec.encode_sessions(slots=5, max_push_samples=4096, sample_rates=(8000, 48000))]
    assert pools[0].cap != pools[1].cap and pools[0].width != pools[1].width
    clips, ref, st = {}, {}, {}
    for k, (fmt, rate, ch, secs, sizes, at, moves) in ENC.items():
        clips[k] = enc_clip(fmt, int(secs * rate) + 7, ch, ord(k), dev)
        mono = pcm.from_g711(clips[k], fmt) if fmt == "ulaw" else (pcm.downmix(clips[k], fmt) if ch > 1 else clips[k])
        ref[k] = codec.encode(mono[None], torch.tensor([mono.shape[0]], device=dev), sample_rate=rate)
        st[k] = dict(at=at, pos=0, i=0, got=[], hops=[], origin=0, done=False)
    for k in ENC:
        fmt, rate, ch = ENC[k][:3]
        st[k]["slot"] = pools[st[k]["at"]].open(sample_rate=rate, sample_format=fmt, channels=ch)

    def hop(k, why):
        s = st[k]
        if ENC[k][6] and why not in s["hops"]:
            s["at"], s["slot"], snap = move(pools, s["at"], s["slot"], dev)
            s["hops"].append(why)
            s["origin"] = pools[s["at"]].origin[s["slot"]]
            s.setdefault("snaps", []).append(snap)

    def one_round(keys):
        named = [{}, {}]
        for k in keys:
            s = st[k]
            if s["done"]:
                continue
            sizes, total = ENC[k][4], clips[k].shape[0]
            n = min(sizes[s["i"] % len(sizes)], total - s["pos"])
            named[s["at"]][k] = clips[k][s["pos"]:s["pos"] + n]
            s["pos"], s["i"] = s["pos"] + n, s["i"] + 1
        for at, chunk in enumerate(named):
            if not chunk:
                continue
            out = pools[at].push({st[k]["slot"]: x for k, x in chunk.items()})
            for k in chunk:
                s = st[k]
                s["got"].append(out[s["slot"]])
                if out[s["slot"]].shape[1] == 0 and s["pos"]:
                    hop(k, "after a push that released no token")
                if pools[s["at"]].origin[s["slot"]] != s["origin"]:
                    s["origin"] = pools[s["at"]].origin[s["slot"]]
                    hop(k, "right after a re-base")
                if s["pos"] == clips[k].shape[0]:
                    hop(k, "before a zero-sample close")
                    s["got"].append(pools[s["at"]].close(s["slot"]))
                    s["done"] = True

    # the neighbours first, one push each: both pools have their buffers (to be filled with NaN) before the first session arrives
    one_round([k for k in ENC if not ENC[k][6]])
    for k in ENC:
        hop(k, "before the first push")
    while not all(s["done"] for s in st.values()):
        one_round(list(ENC))
    _enc.update(ref=ref, st=st, pools=pools)
    return _enc


@pytest.mark.parametrize("clip", list(ENC))
def test_encode_sessions_parked_at_every_point_equal_encode(dev, enc_codec, clip):
    r = encode_run(enc_codec, dev)
    ids, lens = r["ref"][clip]
    mine = torch.cat(r["st"][clip]["got"], dim=1)
    assert int(lens[0]) > 8 and mine.dtype == torch.int32
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    hops = r["st"][clip]["hops"]
    if ENC[clip][6]:
        assert hops[0] == "before the first push" and hops[-1] == "before a zero-sample close"
        assert "after a push that released no token" in hops
        assert ("right after a re-base" in hops) == (clip == "f")
        snaps = r["st"][clip]["snaps"]
        assert snaps[0].nbytes == 0 and all(s.nbytes > 0 for s in snaps[1:])
        assert all(s.meta["kind"] == "encode" and s.meta["rate"] == ENC[clip][1] and s.meta["sample_format"] == ENC[clip][0] for s in snaps)
        assert (snaps[-1].meta["resampler"] is not None) == (ENC[clip][1] != SR)
    else:
        assert hops == []
    assert r["pools"][0].open_slots == [] and r["pools"][1].open_slots == []


# ------------------------------------------------------------------------------------------------------------ decode
# session -> (tokens, open() arguments, push sizes, the pool it starts in, hops: indices of its pushes after which it moves (-1: before
# the first), {index of the push after which the look-ahead moves: its new value})
DEC = {"x": (40, {}, [7, 1, 16, 0, 16], 0, {-1, 0, 1, 3, 4}, {}),
       "e": (38, dict(lookahead_frames=0, crossfade_samples=256), [9, 0, 16, 5, 8], 0, {0, 2, 3}, {2: 8}),
       "r": (30, dict(output_sample_rate=48000, sample_format="s16", channels=2), [16, 3, 0, 11], 0, {-1, 0, 2, 3}, {}),
       "n": (33, dict(lookahead_frames=3), [5, 16, 0, 12], 0, set(), {}),  # neighbours that are never named in park / restore
       "m": (29, {}, [16, 13], 1, set(), {})}
_dec = {}


def dec_clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * F, generator=g).to(dev)
    return ids, noise


def decode_pools(codec):
    opts = dict(early_emit=True, crossfade_samples=256, output_sample_rates=[48000])
    return [codec.decode_sessions(5, max_push_tokens=MAX_PUSH, **opts), codec.decode_sessions(4, max_push_tokens=24, **opts)]


def decode_script(codec, dev, clips, moving):
    """every session of DEC, push by push; moving: the sessions hop between two pools, else all of them live in one pool"""
    pools = decode_pools(codec)
    if not moving:
        pools = [pools[0], pools[0]]
    else:
        assert pools[0].cap != pools[1].cap and pools[0].S != pools[1].S
    st = {k: dict(at=DEC[k][3], slot=pools[DEC[k][3]].open(**DEC[k][1]), pos=0, i=0, got=[], tails=[], snaps=[]) for k in DEC}

    def hop(k, i):
        s = st[k]
        if moving and i in DEC[k][4]:
            s["tails"].append(pools[s["at"]].has_tail[s["slot"]])
            s["at"], s["slot"], snap = move(pools, s["at"], s["slot"], dev)
            s["snaps"].append(snap)

    live = set(DEC)

    def one_round(keys):
        named = [{}, {}] if moving else [{}]
        for k in sorted(keys):
            s, sizes = st[k], DEC[k][2]
            n = min(sizes[s["i"]], DEC[k][0] - s["pos"]) if s["i"] < len(sizes) else 0
            named[s["at"] if moving else 0][k] = (s["pos"], n)
            s["pos"] += n
        for at, plan in enumerate(named):
            if not plan:
                continue
            pool = pools[at]
            final = [k for k in plan if st[k]["i"] >= len(DEC[k][2])]
            out = pool.push({st[k]["slot"]: clips[k][0][:, a:a + n] for k, (a, n) in plan.items()},
                            noise={st[k]["slot"]: clips[k][1][:, F * a:F * (a + n)] for k, (a, n) in plan.items()},
                            final=[st[k]["slot"] for k in final])
            for k in plan:
                s = st[k]
                s["got"].append(out[s["slot"]])
                if k in final:
                    live.discard(k)
                    continue
                if s["i"] in DEC[k][5]:
                    pool.set_lookahead(s["slot"], DEC[k][5][s["i"]])
                hop(k, s["i"])
                s["i"] += 1

    # the neighbours first, one push each: both pools have their buffers (to be filled with NaN) before the first session arrives
    one_round([k for k in DEC if not DEC[k][4]])
    for k in DEC:
        hop(k, -1)
    while live:
        one_round(live & set(DEC))
    assert all(p.open_slots == [] for p in pools)
    return st


def decode_run(codec, dev):
    if not _dec:
        clips = {k: dec_clip(codec, 300 + ord(k), DEC[k][0], dev) for k in DEC}
        _dec.update(clips=clips, plain=decode_script(codec, dev, clips, False), moved=decode_script(codec, dev, clips, True))
    return _dec


@pytest.mark.parametrize("session", list(DEC))
def test_decode_sessions_parked_and_restored_return_every_piece_of_the_uninterrupted_run(dev, dec_codec, session):
    r = decode_run(dec_codec, dev)
    plain, moved = r["plain"][session]["got"], r["moved"][session]["got"]
    assert len(plain) == len(moved) == len(DEC[session][2]) + 1
    for j, ((a0, m0), (a1, m1)) in enumerate(zip(plain, moved)):
        assert a0.dtype == a1.dtype and a0.shape == a1.shape and torch.equal(a0, a1), f"audio piece {j} of session {session}"
        assert torch.equal(m0, m1), f"mel piece {j} of session {session}"
    T = DEC[session][0]
    assert sum(m.shape[1] for _, m in moved) == T * F
    snaps = r["moved"][session]["snaps"]
    assert len(snaps) == len(DEC[session][4])
    if session == "e":                                                      # parked while it holds a tail, and once after set_lookahead
        assert any(r["moved"]["e"]["tails"]) and [s.meta["lookahead"] for s in snaps] == [0, 8, 8]
        assert all(s.meta["fade"] == 256 for s in snaps) and any("fade_tail" in [seg[0] for seg in s.meta["layout"]] for s in snaps)
    if session == "r":
        assert all(s.meta["resampler"]["pair"][1] == 48000 for s in snaps) and moved[0][0].dtype == torch.int16
        assert any("resampler" in [seg[0] for seg in s.meta["layout"]] for s in snaps)
    if session in ("x", "m"):                                               # the exact sessions: decode() of the whole sequence
        ids, noise = r["clips"][session]
        audio, mel = dec_codec.decode(ids[None].contiguous(), torch.tensor([T], device=dev), return_audios=True, noise=noise[None].contiguous())
        assert torch.equal(torch.cat([m for _, m in moved], dim=1), mel[0])
        assert torch.equal(torch.cat([a for a, _ in moved], dim=1), audio[0])


class CountedPack:
    """dmel_stream_pack_items of the bound library wrapped: `calls` grows by one per call"""

    def __enter__(self):
        from dmel_codec_amd import _lib
        self.lib, self.calls = _lib.lib(), 0
        self.inner = self.lib.dmel_stream_pack_items

        def call(*args):
            self.calls += 1
            return self.inner(*args)
        self.lib.dmel_stream_pack_items = call
        return self

    def __exit__(self, *exc):
        self.lib.dmel_stream_pack_items = self.inner


def test_branch_and_one_launch_per_snapshot_and_restore(dev, dec_codec):
    """snapshot without drop, the copy restored into another slot of the SAME pool: two continuations of one reply, each decode()'s"""
    codec = dec_codec
    pool = codec.decode_sessions(4, max_push_tokens=MAX_PUSH)
    base, base_noise = dec_clip(codec, 501, 21, dev)
    tails = [dec_clip(codec, 502 + j, 14 + 5 * j, dev) for j in range(3)]
    with CountedPack() as cp:
        a = pool.open()
        got = {a: [pool.push({a: base[:, :16]}, noise={a: base_noise[:, :64]})[a]]}
        got[a].append(pool.push({a: base[:, 16:]}, noise={a: base_noise[:, 64:]})[a])
        assert cp.calls == 0                                                # none in any push
        snap = pool.snapshot([a])
        assert cp.calls == 1 and pool.open_slots == [a]
        b, c = pool.restore([snap[a], snap[a].to(dev)])
        assert cp.calls == 2 and sorted(pool.open_slots) == sorted([a, b, c]) and len({a, b, c}) == 3
        many = pool.snapshot([c, a, b])                                     # one launch however many slots are named
        assert cp.calls == 3 and all(torch.equal(many[s].blob, snap[a].blob) for s in (a, b, c))
        assert many[a].blob.untyped_storage().data_ptr() == many[c].blob.untyped_storage().data_ptr()       # views of one blob
        for s in (a, b, c):
            got.setdefault(s, list(got[a][:2]))
        for s, (ids, noise) in zip((a, b, c), tails):
            got[s].append(pool.push({s: ids[:, :9]}, noise={s: noise[:, :36]})[s])
        out = pool.push({s: ids[:, 9:] for s, (ids, _) in zip((a, b, c), tails)},
                        noise={s: noise[:, 36:] for s, (_, noise) in zip((a, b, c), tails)}, final=(a, b, c))
        assert cp.calls == 3
    for s, (ids, noise) in zip((a, b, c), tails):
        got[s].append(out[s])
        whole, z = torch.cat([base, ids], dim=1), torch.cat([base_noise, noise], dim=1)
        audio, mel = codec.decode(whole[None].contiguous(), torch.tensor([whole.shape[1]], device=dev), return_audios=True,
                                  noise=z[None].contiguous())
        assert torch.equal(torch.cat([m for _, m in got[s]], dim=1), mel[0]), f"branch in slot {s}"
        assert torch.equal(torch.cat([x for x, _ in got[s]], dim=1), audio[0]), f"branch in slot {s}"
    # a refused restore launches nothing and takes no slot: fewer free slots than snapshots
    with CountedPack() as cp:
        x, y = pool.open(), pool.open()
        pool.push({x: base[:, :9]}, noise={x: base_noise[:, :36]})
        sn = pool.snapshot([x, y])
        z = pool.open()
        with pytest.raises(RuntimeError, match="free"):
            pool.restore(sn)
        assert cp.calls == 1 and sorted(pool.open_slots) == sorted([x, y, z])


def test_a_snapshot_is_bounded_whatever_the_length_of_the_stream(dev, dec_codec):
    codec = dec_codec
    pool = codec.decode_sessions(1, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=256, output_sample_rates=[48000])
    s = pool.open(lookahead_frames=0, crossfade_samples=256, output_sample_rate=48000)
    ids, noise = dec_clip(codec, 77, 40 * MAX_PUSH, dev)
    sizes = {}
    for j in range(40):
        pool.push({s: ids[:, 16 * j:16 * j + 16]}, noise={s: noise[:, 64 * j:64 * j + 64]})
        if j + 1 in (8, 40):
            sizes[j + 1] = pool.snapshot([s])[s].nbytes
    g, dec = pool.geo, codec.decoder
    H, W = g.quant_halo_tokens, g.hold_frames + 1                          # the widest live window: what decode_capacity documents
    rows = (pool.L + 2) * pool.C + dec.condition_channels + dec.output_channels
    bound = 4 * (rows * W + pool.G * 2 * H + pool.C * H * g.factor + 256 + ResampleSchedule(pool.voc_rate, 48000).kw - 1)
    print(f"snapshot of a decode session: {sizes[40]} bytes, bound {bound}")
    assert 0 < sizes[40] <= bound and sizes[40] == sizes[8]
    assert pool.origin[s] > 0                                               # the stream was long enough to be re-based


def test_encode_pool_makes_one_pack_launch_per_snapshot_and_restore(dev, enc_codec):
    """the encode pool's own push path: no pack launch in any push, one per snapshot and one per restore however many slots are named"""
    pool = enc_codec.encode_sessions(slots=4, max_push_samples=2048, sample_rates=(48000,))
    other = enc_codec.encode_sessions(slots=3, max_push_samples=4096, sample_rates=(48000,))
    clips = [enc_clip("f32", 9000, 1, 61, dev), enc_clip("s16", 18000, 2, 62, dev)]
    with CountedPack() as cp:
        slots = [pool.open(), pool.open(sample_rate=48000, sample_format="s16", channels=2)]
        got = [[pool.push({s: x[:2048]})[s]] for s, x in zip(slots, clips)]
        got[0].append(pool.push({slots[0]: clips[0][2048:4096], slots[1]: clips[1][2048:4096]})[slots[0]])
        assert cp.calls == 0
        snaps = pool.park(slots)
        assert cp.calls == 1 and pool.open_slots == []
        moved = other.restore(snaps)
        assert cp.calls == 2 and other.open_slots == moved
        got[0].append(other.push({moved[0]: clips[0][4096:6144], moved[1]: clips[1][4096:6144]})[moved[0]])
        got[0].append(other.push({moved[0]: clips[0][6144:]}, final=(moved[0],))[moved[0]])
        other.drop(moved[1])
        assert cp.calls == 2 and other.open_slots == []
    ids, lens = enc_codec.encode(clips[0][None], torch.tensor([9000], device=dev))
    assert torch.equal(torch.cat(got[0], dim=1), ids[0, :, :int(lens[0])])
