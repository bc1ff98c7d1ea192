"""Streaming decode benchmark (BASELINE.json configs[4], codec side): token ids (1, G, T4) arrive in chunks, audio leaves as soon as its
right context exists (VQGAN.decode_stream: WaveNet state carry + windowed vocoder).  Reports the latency from the first token to the
first audio, the sustained audio-seconds per second at batch 1, and the windowed (stateless, halo re-run) form for comparison.

    python tools/bench_stream.py --output-sample-rate 48000 [--out profiles/stream_resample.txt]

runs only this: two streaming decoders fed the same 64-token chunks, one at the vocoder's rate (output_sample_rate=None) and one with a
StreamResampler behind the vocoder, push i of one followed by push i of the other, each push bracketed by a host synchronisation and timed
on the wall clock; median and 10th / 90th percentile over the steady-state pushes, at batch 1 and 16, APPENDED to --out.

    python tools/bench_stream.py --sessions 16 [--out profiles/decode_sessions.txt]

runs only this: S independent replies whose starts are offset by a third of a push, served (a) by ONE VQGAN.decode_sessions pool step and
(b) by S StreamingDecoder(batch=1) stepped in turn -- what a server could do before the pool existed, so (b) stands for the parent commit.
Both get the same tokens and noise, are interleaved in one process, and every piece of (a) is checked to equal the piece of (b).

    python tools/bench_stream.py --sessions 16 --ragged [--label NAME] [--out profiles/decode_sessions_ragged.txt]

the same with the pushes an LM server makes: every session pushes its own number of tokens in every step, from a seeded list in
[chunk / 2, chunk], so the sessions' mel windows have different lengths in (nearly) every step -- one vocoder pass over all of them in a
pool that has BigVGAN.forward(x, lengths), one pass per group of equal windows in one that has not; the same holds for the token windows
and the quantiser (quantizer.decode(ids, lengths=)).  Both --sessions forms print the quantiser calls per step of the pool.  --label
names the table (the commit measured).

    python tools/bench_stream.py --sessions 16 --output-sample-rate 48000,16000 [--steps 40] [--out profiles/sessions_resample.txt]

runs only this: S replies that leave at the given rates (session i at rate i mod len), served (a) by a pool that was told the rates
(decode_sessions(output_sample_rates=...), open(output_sample_rate=r): ONE resample launch per step) and (b) by the codec-rate pool with
S StreamResampler(batch=1) behind it, one resample launch and two copies per reply: the parent commit's way.  Same tokens and noise,
interleaved in one process, equal audio checked, median and 10th / 90th percentile APPENDED to --out.

    python tools/bench_stream.py --sessions 16 --sample-format s16 [--output-sample-rate 48000,16000] [--steps 40] [--out profiles/sessions_pcm.txt]

runs only this: S replies whose wire carries 16-bit PCM, served (a) by a pool that was told so (open(sample_format="s16"): ONE convert
launch per step into one packed int16 buffer) and (b) by the same pool with f32 sessions and the conversion every caller would do behind
it, `(y * 32768).round().clamp(-32768, 32767).to(int16)` per reply.  With --output-sample-rate the replies also leave at those rates
(both forms).  Same tokens and noise, interleaved in one process, equal audio checked, median and 10th / 90th percentile APPENDED to
--out.

    python tools/bench_stream.py --sessions 16 --sample-format ulaw|alaw --output-sample-rate 8000 [--steps 40] [--out profiles/sessions_g711.txt]

the same for replies whose wire carries G.711 (open(sample_format="ulaw" | "alaw"), torch.uint8 codes, telephony's 8 kHz): (b) is the
same pool with f32 sessions and the companding every caller would do behind it in torch, the s16 rounding and then a clamp / exponent /
shift / xor chain per reply.

    python tools/bench_stream.py --sessions 16 --channels 2 --sample-format s16 [--output-sample-rate 48000] [--steps 40] [--out profiles/sessions_channels.txt]

runs only this: S replies for playback devices opened with C channels, served (a) by a pool that was told so (open(sample_format=...,
channels=C): the ONE convert launch of the step fans every piece out into interleaved frames) and (b) by the same pool with mono
sessions of the same format and what every caller would do behind it, `repeat_interleave(C)` per reply.  Same tokens and noise,
interleaved in one process, equal audio asserted, median and 10th / 90th percentile APPENDED to --out.

    python tools/bench_stream.py --sessions 16 --lookahead 0,8,32 [--push-tokens 1,4,16] [--steps 40] [--out profiles/sessions_early.txt]

runs only this: S replies that emit with bounded look-ahead (decode_sessions(early_emit=True), open(lookahead_frames=K)) against the same
replies in a pool built without early_emit, for every K of the list and every push size: the step time of both (median, p10, p90, p99),
the tokens and stream milliseconds from the first push to the first audio sample (from the schedule), and how far the provisional audio
is from decode()'s (SNR, largest difference at piece boundaries) on the bench's synthetic weights.

    python tools/bench_stream.py --sessions 16 --lookahead 0 --crossfade 256 [--push-tokens 1,4,16] [--steps 40] [--out profiles/sessions_crossfade.txt]

runs only this: S early replies with look-ahead K that cross-fade their pieces over F samples (decode_sessions(early_emit=True,
crossfade_samples=F), open(lookahead_frames=K, crossfade_samples=F)) against the same replies with F = 0, interleaved in one process:
the step time of both, and for session 0 of both the largest sample-to-sample step at the piece boundaries beside the median step of
the stream, on the bench's synthetic weights.

    python tools/bench_stream.py --sessions 16 --park [--steps 40] [--out profiles/sessions_park.txt]

runs only this: S replies in steady state (64-token pushes), then snapshot + restore of all S of them, (a) as the pool does it -- ONE
dmel_stream_pack_items launch per direction -- and (b) with one torch slice .clone() per state tensor per slot and a torch.cat, and
the inverse (tools/bench_park.py): microseconds, bytes moved and GB/s of both, interleaved in one process, APPENDED to --out.

    python tools/bench_stream.py --sessions 16 --tones [--output-sample-rate 8000] [--sample-format ulaw] [--steps 40] [--out profiles/sessions_tones.txt]

runs only this: S replies in steady state (16-token pushes) in three pools interleaved in one process -- decode_sessions() without the
option, decode_sessions(tones=True) with no request due, and the same with a three-key send_dtmf due in every slot in every step: the
step time of each and the launch records of one step ("tones", "small", "pcm_convert"), APPENDED to --out.

    python tools/bench_stream.py --sessions 16 --shape [--output-sample-rate 8000] [--sample-format ulaw] [--steps 40] [--out profiles/sessions_shape.txt]

runs only this: S replies in steady state (16-token pushes) in three pools interleaved in one process -- decode_sessions() without the
option, decode_sessions(shape=True) with no shaping slot, and the same with every slot opened with shape=True at +6 dB: the step time
of each, the launch records of one step ("shape", "small", "pcm_convert") and the time of the dmel_shape_items launch alone, APPENDED
to --out.

    python tools/bench_stream.py --sessions 16 --pace 1250 [--steps 40] [--out profiles/sessions_pace.txt]

runs only this: S replies in steady state (16-token pushes) in three pools interleaved in one process -- decode_sessions() without the
option, decode_sessions(pace=True) with every slot pacing at 1000 (no search), and the same at the given rate (one, or a comma list
assigned round-robin): the step time of each, the launch records of one step ("pace", "small") and, below them, the
dmel_pace_items launch alone on 16384 new samples per slot at 1000 and at the first rate given, dmel_shape_items on the same samples
and one vocoder call of a step's batch for scale, APPENDED to --out."""
import json, math, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

dev = torch.device("cuda:0")
codec = bench.build("cfg2r").to(dev)          # LM configs use the 100-mel / 10-group codec (config/lm/lm_config.yaml)
g = torch.Generator().manual_seed(5)
T4 = 469                                      # 20 s of audio at 23.4 token frames per second
ids = torch.randint(0, 175, (1, 10, T4), generator=g, dtype=torch.int32).to(dev)
flen = torch.tensor([T4], device=dev)
ONLY_PIPE = "--pipeline-only" in sys.argv


def arg_after(flag, default=None):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def output_rate_section(sr, out):
    chunk, warmup, T4L = 64, 6, 64 * 60
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    gl = torch.Generator().manual_seed(6)
    ids_long = torch.randint(0, 175, (1, 10, T4L), generator=gl, dtype=torch.int32).to(dev)
    rows, result = [], {"output_sample_rate": sr, "chunk_tokens": chunk, "batch": {}}
    for B in (1, 16):
        ids_b = ids_long.expand(B, -1, -1).contiguous()
        decs = {"vocoder_rate": codec.streaming_decoder(B, None, True), f"to_{sr}": codec.streaming_decoder(B, None, True, output_sample_rate=sr)}
        ms = {k: [] for k in decs}
        samples = {k: 0 for k in decs}
        keys = list(decs)
        for i, a0 in enumerate(range(0, T4L, chunk)):
            noise = torch.randn(B, codec.decoder.input_channels, chunk * 4, device=dev)
            for k in (keys if i % 2 == 0 else keys[::-1]):                  # neither path always goes first
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a, m = decs[k].push(ids_b[:, :, a0:a0 + chunk], noise=noise)
                torch.cuda.synchronize()
                if i >= warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
                samples[k] += a.shape[-1]
        for k, d in decs.items():
            samples[k] += d.finish()[0].shape[-1]
        r = {"audio_samples": samples}
        for k, v in ms.items():
            med = statistics.median(v)
            r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
            rows.append(f"{B:5d}  {k:12s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
        r["added_median_ms"] = round(r[f"to_{sr}"]["median_ms"] - r["vocoder_rate"]["median_ms"], 3)
        rows.append(f"{B:5d}  conversion adds {r['added_median_ms']:.3f} ms to the median push ({chunk * 4 * 256} vocoder samples per item)")
        result["batch"][str(B)] = r
    table = [f"streaming decode to {sr} Hz, {chunk}-token pushes (2.73 s of audio), 100 mel / 10 groups, BigVGAN base (tools/bench_stream.py --output-sample-rate {sr})",
             f"per-push wall time incl. host synchronisation, {T4L // chunk - warmup} steady-state pushes, the two decoders interleaved in one process;",
             "vocoder_rate = output_sample_rate=None (no resampler), the other = a StreamResampler behind the vocoder",
             "batch  output        median ms     p10 ms     p90 ms     n"] + rows
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_section(S, out, ragged=False, label=""):
    import random
    chunk, warmup, steps = 64, 6, 40
    rng = random.Random(11)
    sizes = [[rng.randint(chunk // 2, chunk) if ragged else chunk for _ in range(S)] for _ in range(steps)]
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    gl = torch.Generator().manual_seed(7)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    total = chunk * (steps + 1)
    ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
    noise = torch.randn(S, Cn, total * 4, device=dev)
    pool = codec.decode_sessions(S, max_push_tokens=chunk)
    slots = [pool.open() for _ in range(S)]
    singles = [codec.streaming_decoder(1, None, True) for _ in range(S)]
    pos = [0] * S
    ms = {"pool": [], "singles": []}

    q_calls, q_decode, calls_per_step = [0], codec.quantizer.decode, []      # quantiser calls of the pool's steps (the counter costs a Python call)

    def counted_decode(*a, **kw):
        q_calls[0] += 1
        return q_decode(*a, **kw)

    def run_pool(n):
        codec.quantizer.decode, q_calls[0] = counted_decode, 0
        out = pool.push({slots[i]: ids[i, :, pos[i]:pos[i] + n[i]] for i in range(S)},
                        noise={slots[i]: noise[i, :, 4 * pos[i]:4 * (pos[i] + n[i])] for i in range(S)})
        del codec.quantizer.decode
        calls_per_step.append(q_calls[0])
        return [out[slots[i]][0] for i in range(S)]

    def run_singles(n):
        return [singles[i].push(ids[i:i + 1, :, pos[i]:pos[i] + n[i]], noise=noise[i:i + 1, :, 4 * pos[i]:4 * (pos[i] + n[i])])[0][0]
                for i in range(S)]

    for step in range(steps):
        # the first push of session i is (i % 3) thirds of a push short, so the sessions' frontiers stay a third of a push apart
        n = [chunk - (i % 3) * (chunk // 3) if step == 0 and not ragged else sizes[step][i] for i in range(S)]
        got = {}
        for k, fn in ((("pool", run_pool), ("singles", run_singles)) if step % 2 == 0 else (("singles", run_singles), ("pool", run_pool))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = fn(n)
            torch.cuda.synchronize()
            if step >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for i in range(S):
            assert torch.equal(got["pool"][i], got["singles"][i]), f"step {step}, session {i}: the pool's audio differs"
            pos[i] += n[i]
    audio_s = statistics.mean(sum(n) for n in sizes[warmup:]) * 4 * 256 / 24000      # of a steady-state step, all sessions
    rows, result = [], {"sessions": S, "chunk_tokens": chunk, "ragged": ragged, "label": label,
                        "quantizer_calls_per_step": {"mean": round(statistics.mean(calls_per_step[warmup:]), 2), "max": max(calls_per_step[warmup:])}}
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                     "audio_sec_per_sec": round(audio_s / (med * 1e-3), 1)}
        rows.append(f"{S:8d}  {k:8s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  {audio_s / (med * 1e-3):10.1f}")
    result["speedup_median"] = round(result["singles"]["median_ms"] / result["pool"]["median_ms"], 3)
    pushes = f"pushes of {chunk // 2}..{chunk} tokens, another size per session and step (seeded)" if ragged else \
        f"{chunk}-token pushes, starts a third of a push apart"
    table = [(f"[{label}] " if label else "") + f"{S} independent decode sessions, {pushes}, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S}" + (" --ragged)" if ragged else ")"),
             f"wall time of one step of all sessions incl. host synchronisation, {steps - warmup} steady-state steps, the two interleaved in one process, "
             "equal audio checked;",
             "pool = one VQGAN.decode_sessions step; singles = S StreamingDecoder(batch=1) pushed in turn (the parent commit's way)",
             "sessions  served by  median ms     p10 ms     p90 ms     n  audio-s / s"] + rows + [
                 f"pool / singles: {result['speedup_median']:.3f}x at the median",
                 f"quantiser calls per pool step: mean {result['quantizer_calls_per_step']['mean']:.2f}, max {result['quantizer_calls_per_step']['max']}"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_rates_section(S, rates, steps, out):
    from dmel_codec_amd.utils.resample import StreamResampler
    chunk, warmup = 64, 6
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    gl = torch.Generator().manual_seed(8)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    total = chunk * (steps + 1)
    ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
    noise = torch.randn(S, Cn, total * 4, device=dev)
    rate = [rates[i % len(rates)] for i in range(S)]
    pool = codec.decode_sessions(S, max_push_tokens=chunk, output_sample_rates=rates)
    slots = [pool.open(output_sample_rate=rate[i]) for i in range(S)]
    plain = codec.decode_sessions(S, max_push_tokens=chunk)
    pslots = [plain.open() for _ in range(S)]
    behind = [StreamResampler(pool.voc_rate, rate[i], 1) for i in range(S)]
    pos = [0] * S
    ms = {"per_slot_rates": [], "resamplers_behind": []}

    def feed(sl, n):
        return ({sl[i]: ids[i, :, pos[i]:pos[i] + n[i]] for i in range(S)},
                {sl[i]: noise[i, :, 4 * pos[i]:4 * (pos[i] + n[i])] for i in range(S)})

    def run_pool(n):
        t, z = feed(slots, n)
        out = pool.push(t, noise=z)
        return [out[slots[i]][0] for i in range(S)]

    def run_behind(n):
        t, z = feed(pslots, n)
        out = plain.push(t, noise=z)
        return [behind[i].push(out[pslots[i]][0]) for i in range(S)]

    for step in range(steps):
        n = [chunk - (i % 3) * (chunk // 3) if step == 0 else chunk for i in range(S)]
        got = {}
        order = (("per_slot_rates", run_pool), ("resamplers_behind", run_behind))
        for k, fn in (order if step % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = fn(n)
            torch.cuda.synchronize()
            if step >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for i in range(S):
            assert torch.equal(got["per_slot_rates"][i], got["resamplers_behind"][i]), f"step {step}, session {i}: the pool's audio differs"
            pos[i] += n[i]
    rows, result = [], {"sessions": S, "output_sample_rates": rates, "chunk_tokens": chunk, "audio_equal": True}
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:17s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    result["behind_over_per_slot"] = round(result["resamplers_behind"]["median_ms"] / result["per_slot_rates"]["median_ms"], 3)
    rl = ",".join(map(str, rates))
    table = [f"{S} decode sessions leaving at {rl} Hz, {chunk}-token pushes, starts a third of a push apart, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S} --output-sample-rate {rl})",
             f"wall time of one step of all sessions incl. host synchronisation, {steps - warmup} steady-state steps, the two interleaved in one process, "
             "equal audio checked;",
             "per_slot_rates = decode_sessions(output_sample_rates=...): one resample launch per step; resamplers_behind = the codec-rate pool "
             "with one StreamResampler(batch=1) per session behind it",
             "sessions  form               median ms     p10 ms     p90 ms     n"] + rows + [
                 f"resamplers behind / per-slot rates: {result['behind_over_per_slot']:.3f} at the median"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def torch_g711(y, law):
    """what a caller without G.711 sessions runs behind every reply: the s16 rounding, then the companding rule of utils/pcm.py in
    torch integer ops (the segment from the float exponent, which is exact)"""
    x = (y * 32768).round().clamp(-32768, 32767).to(torch.int32)
    v = x >> (2 if law == "ulaw" else 3)
    neg = v < 0
    if law == "ulaw":
        m = (torch.where(neg, -v, v) + 33).clamp(max=8191)
        seg = torch.frexp(m.float())[1] - 6
        code = ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ torch.where(neg, 0x7F, 0xFF)
    else:
        m = torch.where(neg, -v - 1, v)
        seg = (torch.frexp(m.clamp(min=1).float())[1] - 5).clamp(min=0)
        code = ((seg << 4) | ((m >> seg.clamp(min=1)) & 15)) ^ torch.where(neg, 0x55, 0xD5)
    return code.to(torch.uint8)


def sessions_pcm_section(S, rates, steps, out, fmt="s16"):
    chunk, warmup = 64, 6
    wire, wire_dtype = f"{fmt}_sessions", torch.int16 if fmt == "s16" else torch.uint8
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    gl = torch.Generator().manual_seed(9)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    total = chunk * (steps + 1)
    ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
    noise = torch.randn(S, Cn, total * 4, device=dev)
    rate = [rates[i % len(rates)] if rates else None for i in range(S)]
    pools = {wire: codec.decode_sessions(S, max_push_tokens=chunk, output_sample_rates=rates),
             "torch_behind": codec.decode_sessions(S, max_push_tokens=chunk, output_sample_rates=rates)}
    slots = {wire: [pools[wire].open(output_sample_rate=rate[i], sample_format=fmt) for i in range(S)],
             "torch_behind": [pools["torch_behind"].open(output_sample_rate=rate[i]) for i in range(S)]}
    pos = [0] * S
    ms = {k: [] for k in pools}

    def run(k, n):
        sl = slots[k]
        out = pools[k].push({sl[i]: ids[i, :, pos[i]:pos[i] + n[i]] for i in range(S)},
                            noise={sl[i]: noise[i, :, 4 * pos[i]:4 * (pos[i] + n[i])] for i in range(S)})
        if k == wire:
            return [out[sl[i]][0] for i in range(S)]
        if fmt != "s16":
            return [torch_g711(out[sl[i]][0], fmt) for i in range(S)]
        return [(out[sl[i]][0] * 32768).round().clamp(-32768, 32767).to(torch.int16) for i in range(S)]

    for step in range(steps):
        n = [chunk - (i % 3) * (chunk // 3) if step == 0 else chunk for i in range(S)]
        got = {}
        keys = list(ms)
        for k in (keys if step % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = run(k, n)
            torch.cuda.synchronize()
            if step >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for i in range(S):
            assert got[wire][i].dtype == wire_dtype and torch.equal(got[wire][i], got["torch_behind"][i]), \
                f"step {step}, session {i}: the pool's audio differs"
            pos[i] += n[i]
    rows, result = [], {"sessions": S, "sample_format": fmt, "output_sample_rates": rates, "chunk_tokens": chunk, "audio_equal": True}
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:13s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    result[f"torch_over_{fmt}"] = round(result["torch_behind"]["median_ms"] / result[wire]["median_ms"], 3)
    rl = ",".join(map(str, rates)) if rates else "the vocoder's rate"
    name = {"s16": "16-bit PCM", "ulaw": "G.711 mu-law", "alaw": "G.711 A-law"}[fmt]
    table = [f"{S} decode sessions returning {name} at {rl}, {chunk}-token pushes, starts a third of a push apart, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S} --sample-format {fmt}" + (f" --output-sample-rate {rl})" if rates else ")"),
             f"wall time of one step of all sessions incl. host synchronisation, {steps - warmup} steady-state steps, the two interleaved in one process, "
             "equal audio checked;",
             f"{wire} = open(sample_format=\"{fmt}\"): one convert launch per step; torch_behind = f32 sessions, " +
             ("(y * 32768).round().clamp().to(int16) per reply" if fmt == "s16" else
              "the s16 rounding and a clamp / exponent / shift / xor chain in torch per reply"),
             "sessions  form           median ms     p10 ms     p90 ms     n"] + rows + [
                 f"torch behind / {fmt} sessions: {result[f'torch_over_{fmt}']:.3f} at the median"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_channels_section(S, rates, steps, out, fmt, ch):
    chunk, warmup = 64, 6
    wire = f"{ch}ch_sessions"
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    gl = torch.Generator().manual_seed(10)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    total = chunk * (steps + 1)
    ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
    noise = torch.randn(S, Cn, total * 4, device=dev)
    rate = [rates[i % len(rates)] if rates else None for i in range(S)]
    pools = {wire: codec.decode_sessions(S, max_push_tokens=chunk, output_sample_rates=rates),
             "torch_behind": codec.decode_sessions(S, max_push_tokens=chunk, output_sample_rates=rates)}
    slots = {wire: [pools[wire].open(output_sample_rate=rate[i], sample_format=fmt, channels=ch) for i in range(S)],
             "torch_behind": [pools["torch_behind"].open(output_sample_rate=rate[i], sample_format=fmt) for i in range(S)]}
    pos = [0] * S
    ms = {k: [] for k in pools}

    def run(k, n):
        sl = slots[k]
        out = pools[k].push({sl[i]: ids[i, :, pos[i]:pos[i] + n[i]] for i in range(S)},
                            noise={sl[i]: noise[i, :, 4 * pos[i]:4 * (pos[i] + n[i])] for i in range(S)})
        if k == wire:
            return [out[sl[i]][0] for i in range(S)]
        return [out[sl[i]][0][0].repeat_interleave(ch).view(-1, ch) for i in range(S)]

    for step in range(steps):
        n = [chunk - (i % 3) * (chunk // 3) if step == 0 else chunk for i in range(S)]
        got = {}
        keys = list(ms)
        for k in (keys if step % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = run(k, n)
            torch.cuda.synchronize()
            if step >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for i in range(S):
            a, b = got[wire][i], got["torch_behind"][i]
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), \
                f"step {step}, session {i}: the pool's audio differs"
            pos[i] += n[i]
    rows, result = [], {"sessions": S, "channels": ch, "sample_format": fmt, "output_sample_rates": rates, "chunk_tokens": chunk,
                        "audio_equal": True, "runs": 1}
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:13s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    result["torch_over_channels"] = round(result["torch_behind"]["median_ms"] / result[wire]["median_ms"], 3)
    rl = ",".join(map(str, rates)) if rates else "the vocoder's rate"
    table = [f"{S} decode sessions returning interleaved {ch}-channel {fmt} frames at {rl}, {chunk}-token pushes, starts a third of a push apart, "
             f"100 mel / 10 groups, BigVGAN base (tools/bench_stream.py --sessions {S} --channels {ch} --sample-format {fmt}" +
             (f" --output-sample-rate {rl})" if rates else ")"),
             f"wall time of one step of all sessions incl. host synchronisation, {steps - warmup} steady-state steps, the two interleaved in one process, "
             "equal audio asserted;",
             f"{wire} = open(sample_format=\"{fmt}\", channels={ch}): one convert launch per step, the fan-out inside it; torch_behind = mono {fmt} "
             f"sessions, repeat_interleave({ch}) per reply",
             "sessions  form           median ms     p10 ms     p90 ms     n"] + rows + [
                 f"torch behind / {ch}-channel sessions: {result['torch_over_channels']:.3f} at the median; one run"]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_early_section(S, lookaheads, pushes, steps, out, label=""):
    """early against exact sessions: S replies pushed `p` tokens per step, served by a pool built without early_emit (today's path) and by
    one built with it whose sessions were opened with lookahead_frames=k; the two interleaved in one process"""
    from dmel_codec_amd.models.stream_schedule import DecodeSchedule, EarlyDecodeSchedule
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    rows, results = [], []
    for p in pushes:
        for k in lookaheads:
            pools = {"exact": codec.decode_sessions(S, max_push_tokens=max(pushes)),
                     f"early_k{k}": codec.decode_sessions(S, max_push_tokens=max(pushes), early_emit=True)}
            early = f"early_k{k}"
            geo = pools["exact"].geo
            hold_tokens = -(-geo.hold_frames // geo.factor)
            warmup = max(6, hold_tokens // p + 3)                     # the early path re-decodes up to the hold: steady only behind it
            total = p * (warmup + steps)
            gl = torch.Generator().manual_seed(12)
            ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
            noise = torch.randn(S, Cn, total * 4, generator=gl).to(dev)
            slots = {"exact": [pools["exact"].open() for _ in range(S)], early: [pools[early].open(lookahead_frames=k) for _ in range(S)]}
            ms = {name: [] for name in pools}
            pieces = []                                               # session 0 of the early pool
            for step in range(warmup + steps):
                a = p * step
                names = list(pools)
                for name in (names if step % 2 == 0 else names[::-1]):
                    sl = slots[name]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = pools[name].push({sl[i]: ids[i, :, a:a + p] for i in range(S)},
                                           noise={sl[i]: noise[i, :, 4 * a:4 * (a + p)] for i in range(S)})
                    torch.cuda.synchronize()
                    if step >= warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                    if name == early:
                        pieces.append(got[sl[0]][0])
            for name, pool in pools.items():
                for i, s in enumerate(slots[name]):
                    last = pool.close(s)
                    if name == early and i == 0:
                        pieces.append(last[0])
            # (c) how far the provisional audio is from decode()'s, on these synthetic weights
            ref = codec.decode(ids[:1], torch.tensor([total], device=dev), return_audios=True, noise=noise[:1])[0][0]
            mine = torch.cat(pieces, dim=1)
            assert mine.shape == ref.shape, (mine.shape, ref.shape)
            d = (mine - ref).double()
            err = float((d * d).sum())
            snr = float("inf") if err == 0 else 10 * math.log10(float((ref.double() ** 2).sum()) / err)
            cuts, at = [], 0
            for piece in pieces[:-1]:
                at += piece.shape[1]
                if 0 < at < ref.shape[1]:
                    cuts += [at - 1, at]
            edge = float(d[0, sorted(set(cuts))].abs().max()) if cuts else 0.0
            # (b) first audio: from the schedule, in tokens received and in the stream time they stand for
            first = {}
            for name, sch in (("exact", DecodeSchedule(geo)), (early, EarlyDecodeSchedule(geo, k))):
                n = 0
                while True:
                    n += p
                    if sch.step(p).emit[1] > 0:
                        break
                first[name] = n
            tok_s = 24000 / (256 * geo.factor)
            r = {"push_tokens": p, "lookahead_frames": k, "snr_db": round(snr, 2) if snr != float("inf") else "inf",
                 "max_abs_diff_at_piece_boundaries": edge, "peak": float(ref.abs().max())}
            for name, v in ms.items():
                med = statistics.median(v)
                r[name] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3),
                           "p99_ms": round(pct(v, 0.99), 3), "n": len(v), "first_audio_after_tokens": first[name],
                           "first_audio_after_ms": round(first[name] / tok_s * 1e3, 1)}
                rows.append(f"{p:4d}  {name:11s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {pct(v, 0.99):9.3f}  {len(v):4d}  "
                            f"{first[name]:6d}  {first[name] / tok_s * 1e3:8.1f}" +
                            (f"  {r['snr_db']:>7}  {edge:9.2e}" if name == early else ""))
            results.append(r)
    table = [(f"[{label}] " if label else "") + f"{S} decode sessions, early against exact, pushes of {','.join(map(str, pushes))} tokens, 100 mel / 10 groups, "
             f"BigVGAN base (tools/bench_stream.py --sessions {S} --lookahead {','.join(map(str, lookaheads))})",
             f"wall time of one step of all sessions incl. host synchronisation, {steps} steady-state steps, the two pools interleaved in one process;",
             "exact = a pool built without early_emit; early_kK = decode_sessions(early_emit=True), every session open(lookahead_frames=K);",
             "first audio: tokens received, and the stream time they stand for, when the first sample leaves -- from the schedule, not a timer;",
             "SNR / edge: session 0's concatenated early audio against decode()'s, edge = largest |difference| one sample either side of a piece "
             "boundary.  SYNTHETIC weights: this says nothing about a trained checkpoint",
             "push  pool         median ms     p10 ms     p90 ms     p99 ms     n  first: tokens    ms   SNR dB       edge"] + rows
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps({"sessions": S, "label": label, "results": results}))


def sessions_crossfade_section(S, k, fade, pushes, steps, out, label=""):
    """cross-fading against plain early sessions: S replies pushed `p` tokens per step with look-ahead k, served by a pool built with
    crossfade_samples=fade whose sessions were opened with it and by the same pool with F = 0; the two interleaved in one process.
    For session 0 of both: the sample-to-sample step |x[i + 1] - x[i]| of the concatenated audio across the pool's own piece
    boundaries (`fade` samples earlier with the fade), over the `fade` samples in front of every raw boundary -- the blended region
    of one pool, the same samples and the raw cut behind them in the other -- and its median and 99th percentile everywhere"""
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    rows, results = [], []
    for p in pushes:
        pools = {"early_F0": codec.decode_sessions(S, max_push_tokens=max(pushes), early_emit=True),
                 f"fade_F{fade}": codec.decode_sessions(S, max_push_tokens=max(pushes), early_emit=True, crossfade_samples=fade)}
        plain, faded = list(pools)
        geo, up = pools[plain].geo, pools[plain].up
        warmup = max(6, -(-geo.hold_frames // geo.factor) // p + 3)
        total = p * (warmup + steps)
        gl = torch.Generator().manual_seed(12)
        ids = torch.randint(0, 175, (S, G, total), generator=gl, dtype=torch.int32).to(dev)
        noise = torch.randn(S, Cn, total * 4, generator=gl).to(dev)
        slots = {plain: [pools[plain].open(lookahead_frames=k) for _ in range(S)],
                 faded: [pools[faded].open(lookahead_frames=k, crossfade_samples=fade) for _ in range(S)]}
        ms = {name: [] for name in pools}
        pieces = {name: [] for name in pools}                         # session 0 of each pool
        frames = []                                                   # the mel frames session 0 has handed out after every push
        for step in range(warmup + steps):
            a = p * step
            names = list(pools)
            for name in (names if step % 2 == 0 else names[::-1]):
                sl = slots[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = pools[name].push({sl[i]: ids[i, :, a:a + p] for i in range(S)},
                                       noise={sl[i]: noise[i, :, 4 * a:4 * (a + p)] for i in range(S)})
                torch.cuda.synchronize()
                if step >= warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                pieces[name].append(got[sl[0]][0])
                if name == plain:
                    frames.append(pools[name].frames_emitted(sl[0]))
        for name, pool in pools.items():
            for i, s in enumerate(slots[name]):
                last = pool.close(s)
                if i == 0:
                    pieces[name].append(last[0])
        cuts = sorted({f * up for f in frames if 0 < f * up < total * geo.factor * up})    # the raw piece boundaries, in samples
        r = {"push_tokens": p, "lookahead_frames": k, "crossfade_samples": fade, "piece_boundaries": len(cuts)}
        for name in pools:
            x = torch.cat(pieces[name], dim=1)[0].double()
            assert x.shape[0] == total * geo.factor * up, (name, x.shape)
            d = (x[1:] - x[:-1]).abs()                                # d[i]: the step from sample i to sample i + 1
            own = torch.tensor([c - 1 - (fade if name == faded else 0) for c in cuts], device=dev)
            near = torch.tensor(sorted({i for c in cuts for i in range(max(0, c - fade - 1), c)}), device=dev)
            edge, region = (float(d[own].max()), float(d[near].max())) if cuts else (0.0, 0.0)
            v = ms[name]
            med = statistics.median(v)
            r[name] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3),
                       "p99_ms": round(pct(v, 0.99), 3), "n": len(v), "max_step_across_piece_boundaries": edge,
                       "max_step_in_the_fade_regions": region,
                       "median_step": float(d.median()), "p99_step": float(d.quantile(0.99)), "peak": float(x.abs().max())}
            rows.append(f"{p:4d}  {name:11s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {pct(v, 0.99):9.3f}  {len(v):4d}  "
                        f"{len(cuts):5d}  {edge:9.2e}  {region:9.2e}  {float(d.median()):9.2e}  {float(d.quantile(0.99)):9.2e}  {float(x.abs().max()):6.3f}")
        results.append(r)
    table = [(f"[{label}] " if label else "") + f"{S} early decode sessions, look-ahead {k} frames, cross-fade {fade} samples against none, pushes of "
             f"{','.join(map(str, pushes))} tokens, 100 mel / 10 groups, BigVGAN base (tools/bench_stream.py --sessions {S} --lookahead {k} "
             f"--crossfade {fade})",
             f"wall time of one step of all sessions incl. host synchronisation, {steps} steady-state steps, the two pools interleaved in one process;",
             f"early_F0 = decode_sessions(early_emit=True), every session open(lookahead_frames={k}); fade_F{fade} = the same with "
             f"crossfade_samples={fade} at the pool and at every open: one cross-fade launch more per step;",
             "step = |x[i + 1] - x[i]| of session 0's concatenated audio: `boundary` its largest value across the pool's own piece boundaries (one "
             f"step per piece), `region` over the {fade} samples in front of every raw boundary and the step behind them (the blended samples of the "
             "fading pool; the same samples and the raw cut in the other), median / p99 over the whole stream.",
             "SYNTHETIC weights: this says nothing about a trained checkpoint",
             "push  pool         median ms     p10 ms     p90 ms     p99 ms     n   cuts   boundary     region  median st     p99 st    peak"] + rows
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps({"sessions": S, "label": label, "results": results}))


if "--crossfade" in sys.argv:
    assert "--sessions" in sys.argv and "--lookahead" in sys.argv, "--crossfade needs --sessions and --lookahead K"
    sessions_crossfade_section(int(arg_after("--sessions")), int(arg_after("--lookahead")), int(arg_after("--crossfade")),
                               [int(p) for p in arg_after("--push-tokens", "1,4,16").split(",")], int(arg_after("--steps", "40")),
                               arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                               "sessions_crossfade.txt")), arg_after("--label", ""))
    sys.exit(0)

def sessions_park_section(S, steps, out):
    import bench_park
    chunk, pushes = 64, 8
    gl = torch.Generator().manual_seed(7)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    ids = torch.randint(0, 175, (S, G, chunk * pushes), generator=gl, dtype=torch.int32).to(dev)
    pool = codec.decode_sessions(S, max_push_tokens=chunk)
    slots = [pool.open() for _ in range(S)]
    for j in range(pushes):                                                  # steady state: every slot holds its widest window
        pool.push({s: ids[i, :, j * chunk:(j + 1) * chunk] for i, s in enumerate(slots)},
                  noise={s: torch.randn(Cn, chunk * 4, device=dev) for s in slots})
    result, rows, slots = bench_park.measure(pool, slots, reps=steps)
    table = [f"snapshot + restore of {S} decode sessions in steady state ({chunk}-token pushes), 100 mel / 10 groups, {pool.L} decoder layers of "
             f"{pool.C} channels, cap {pool.cap} (tools/bench_stream.py --sessions {S} --park)",
             f"wall time of one snapshot of all sessions and one restore of all of them incl. host synchronisation, {result['cycles']} cycles, the two "
             "interleaved in one process, equal words checked;",
             "one_launch = pool.park + pool.restore (ONE dmel_stream_pack_items launch each); torch_slices = a slice .clone() per tensor per slot "
             "and a cat, and a slice copy per tensor back",
             "sessions  way            median us      p10 us      p90 us     n  bytes moved      GB/s"] + rows
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_tones_section(S, rate, fmt, steps, out):
    from dmel_codec_amd import _lib
    chunk, warmup = 16, 8
    gl = torch.Generator().manual_seed(8)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    n_steps = warmup + steps
    ids = torch.randint(0, 175, (S, G, chunk * n_steps), generator=gl, dtype=torch.int32).to(dev)
    kw = dict(max_push_tokens=chunk, output_sample_rates=(rate,) if rate else ())
    open_kw = dict(output_sample_rate=rate or None, sample_format=fmt)
    pools = {"no_tones_pool": codec.decode_sessions(S, **kw), "tones_pool_idle": codec.decode_sessions(S, tones=True, **kw),
             "tones_pool_3_keys": codec.decode_sessions(S, tones=True, **kw)}
    slots = {k: [p.open(**open_kw) for _ in range(S)] for k, p in pools.items()}
    ms, launches, samples = {k: [] for k in pools}, {k: {} for k in pools}, {k: 0 for k in pools}
    keys, families = list(pools), ("tones", "small", "pcm_convert")
    for j in range(n_steps):
        noise = [torch.randn(Cn, chunk * 4, device=dev) for _ in range(S)]
        counted = j == n_steps - 1                                          # the launch records of the last step, which is not timed
        for k in (keys if j % 2 == 0 else keys[::-1]):                      # no pool always goes first
            pool = pools[k]
            if k == "tones_pool_3_keys":                                    # at the newest frame every slot has handed out: due in this step
                for s in slots[k]:
                    pool.send_dtmf(s, "159", at_frame=pool.frames_emitted(s))
            if counted:
                _lib.prof_reset(); _lib.prof_enable(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.push({s: ids[i, :, j * chunk:(j + 1) * chunk] for i, s in enumerate(slots[k])},
                            noise={s: noise[i] for i, s in enumerate(slots[k])})
            torch.cuda.synchronize()
            if counted:
                launches[k] = {f: _lib.prof_read(f)["launches"] for f in families}
                _lib.prof_enable(False); _lib.prof_reset()
            elif j >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            samples[k] += sum(a.numel() for a, _ in res.values())
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    result, rows = {"sessions": S, "chunk_tokens": chunk, "output_sample_rate": rate or pools[keys[0]].voc_rate, "sample_format": fmt}, []
    for k in keys:
        v = ms[k]
        result[k] = {"median_ms": round(statistics.median(v), 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                     "launches_per_step": launches[k], "audio_samples": samples[k]}
        rows.append(f"{S:8d}  {k:18s}  {statistics.median(v):9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  "
                    f"{launches[k]['tones']:5d}  {launches[k]['small']:5d}  {launches[k]['pcm_convert']:11d}")
    # a difference is a cost only where the medians leave each other's p10 .. p90; inside it the pools are level
    med = [result[k]["median_ms"] for k in keys]
    level = all(result[k]["p10_ms"] <= m <= result[k]["p90_ms"] for k in keys for m in med)
    result["level_within_spread"] = level
    verdict = (f"the three medians lie inside each other's p10 .. p90: level within spread, no cost of the option or of the tone step "
               f"({S} slots, three keys each) is resolved" if level else
               f"medians outside each other's p10 .. p90: idle tone pool {med[1] - med[0]:+.3f} ms against the pool without the option, "
               f"tone step {med[2] - med[1]:+.3f} ms against the idle tone pool (new work: no threshold)")
    table = [f"{S} decode sessions, {chunk}-token pushes, audio at {result['output_sample_rate']} Hz as {fmt}, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S} --tones)",
             f"per-step wall time incl. host synchronisation, {steps} steady-state steps, the three pools interleaved in one process;",
             "no_tones_pool = decode_sessions() as it was; tones_pool_idle = decode_sessions(tones=True), no request due; tones_pool_3_keys = "
             "the same with send_dtmf(slot, '159') due in every slot in every step (11520 samples of tones per slot and step)",
             "launch records of one step: tones (dmel_tone_items), small (all small kernels, the tone launch among them), pcm_convert",
             "sessions  pool                median ms     p10 ms     p90 ms     n  tones  small  pcm_convert"] + rows + [
             verdict]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


if "--tones" in sys.argv:
    assert "--sessions" in sys.argv, "--tones needs --sessions"
    sessions_tones_section(int(arg_after("--sessions")), int(arg_after("--output-sample-rate", "0")), arg_after("--sample-format", "f32"),
                           int(arg_after("--steps", "40")),
                           arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                           "sessions_tones.txt")))
    sys.exit(0)

def sessions_shape_section(S, rate, fmt, steps, out):
    """three pools interleaved in one process: decode_sessions() as it was, decode_sessions(shape=True) with no shaping slot, and the
    same with every slot opened with shape=True at +6 dB (the limiter works); below them the shape launch alone"""
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import shape as shape_rule
    chunk, warmup = 16, 8
    gl = torch.Generator().manual_seed(8)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    n_steps = warmup + steps
    ids = torch.randint(0, 175, (S, G, chunk * n_steps), generator=gl, dtype=torch.int32).to(dev)
    kw = dict(max_push_tokens=chunk, output_sample_rates=(rate,) if rate else ())
    open_kw = dict(output_sample_rate=rate or None, sample_format=fmt)
    pools = {"no_shape_pool": codec.decode_sessions(S, **kw), "shape_pool_idle": codec.decode_sessions(S, shape=True, **kw),
             "shape_pool_all": codec.decode_sessions(S, shape=True, **kw)}
    slots = {k: [p.open(**open_kw, **(dict(shape=True) if k == "shape_pool_all" else {})) for _ in range(S)] for k, p in pools.items()}
    for s in slots["shape_pool_all"]:
        pools["shape_pool_all"].set_gain(s, 6.0, ramp_ms=20.0)
    ms, launches, samples = {k: [] for k in pools}, {k: {} for k in pools}, {k: 0 for k in pools}
    keys, families = list(pools), ("shape", "small", "pcm_convert")
    for j in range(n_steps):
        noise = [torch.randn(Cn, chunk * 4, device=dev) for _ in range(S)]
        counted = j == n_steps - 1                                          # the launch records of the last step, which is not timed
        for k in (keys if j % 2 == 0 else keys[::-1]):                      # no pool always goes first
            pool = pools[k]
            if counted:
                _lib.prof_reset(); _lib.prof_enable(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.push({s: ids[i, :, j * chunk:(j + 1) * chunk] for i, s in enumerate(slots[k])},
                            noise={s: noise[i] for i, s in enumerate(slots[k])})
            torch.cuda.synchronize()
            if counted:
                launches[k] = {f: _lib.prof_read(f)["launches"] for f in families}
                _lib.prof_enable(False); _lib.prof_reset()
            elif j >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            samples[k] += sum(a.numel() for a, _ in res.values())
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    result, rows = {"sessions": S, "chunk_tokens": chunk, "output_sample_rate": rate or pools[keys[0]].voc_rate, "sample_format": fmt}, []
    for k in keys:
        v = ms[k]
        result[k] = {"median_ms": round(statistics.median(v), 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                     "launches_per_step": launches[k], "audio_samples": samples[k]}
        rows.append(f"{S:8d}  {k:18s}  {statistics.median(v):9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  "
                    f"{launches[k]['shape']:5d}  {launches[k]['small']:5d}  {launches[k]['pcm_convert']:11d}")
    reports = pools["shape_pool_all"].shaped()
    result["limited_blocks"] = sum(r.limited_blocks for r in reports.values())
    # the launch alone: S slots, one step's samples each, fresh rows every time
    cfg, n = shape_rule.ShapeConfig(), chunk * 4 * pools[keys[0]].up
    vr = pools[keys[0]].voc_rate
    x = (torch.randn(S, n, device=dev) * 0.5).contiguous()
    y = torch.empty(S, n + 2 * shape_rule.MAX_BLOCK, device=dev)
    st = torch.zeros(S, cfg.state_words(vr), dtype=torch.int32, device=dev)
    pk, gn = torch.zeros(S, n // 32 + 2, device=dev), torch.zeros(S, n // 32 + 2, device=dev)
    tab = torch.empty(shape_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    ramps, off = shape_rule.ramp_arena([480], dev)
    alone = []
    for j in range(warmup + steps):
        st.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shape_rule.shape_items([x[s] for s in range(S)], [y[s] for s in range(S)], [cfg] * S, [[(0, 1.0, 2.0, 480)]] * S, [1.0] * S, [0] * S,
                               [0] * S, [False] * S, st, pk, gn, vr, ramps=ramps, ramp_off=off, table=tab)
        torch.cuda.synchronize()
        if j >= warmup:
            alone.append((time.perf_counter() - t0) * 1e3)
    result["launch_alone"] = {"median_ms": round(statistics.median(alone), 4), "p10_ms": round(pct(alone, 0.1), 4),
                              "p90_ms": round(pct(alone, 0.9), 4), "samples_per_slot": n}
    med = [result[k]["median_ms"] for k in keys]
    level = all(result[k]["p10_ms"] <= m <= result[k]["p90_ms"] for k in keys[:2] for m in med[:2])
    result["idle_level_within_spread"] = level
    verdict = (("the pool without the option and the shape pool without a shaping slot lie inside each other's p10 .. p90: level within "
                "spread" if level else f"shape pool without a shaping slot {med[1] - med[0]:+.3f} ms against the pool without the option, outside "
                "the spread") + f"; every slot shaping {med[2] - med[0]:+.3f} ms against the pool without the option (new work: no threshold)")
    table = [f"{S} decode sessions, {chunk}-token pushes, audio at {result['output_sample_rate']} Hz as {fmt}, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S} --shape)",
             f"per-step wall time incl. host synchronisation, {steps} steady-state steps, the three pools interleaved in one process;",
             "no_shape_pool = decode_sessions() as it was; shape_pool_idle = decode_sessions(shape=True), no slot opened with shape=; "
             "shape_pool_all = the same with every slot opened with shape=True and set_gain(+6 dB)",
             "launch records of one step: shape (dmel_shape_items), small (all small kernels, the shape launch among them), pcm_convert",
             "sessions  pool                median ms     p10 ms     p90 ms     n  shape  small  pcm_convert"] + rows + [
             f"dmel_shape_items alone, {S} slots of {n} samples, fresh rows, wall time incl. host synchronisation: median "
             f"{statistics.median(alone):.4f} ms, p10 {pct(alone, 0.1):.4f}, p90 {pct(alone, 0.9):.4f}; limited blocks over the run: "
             f"{result['limited_blocks']}", verdict]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def sessions_pace_section(S, rates, steps, out):
    """three pools interleaved in one process: decode_sessions() as it was, decode_sessions(pace=True) with every slot pacing at 1000,
    and the same with the slots at `rates`, round-robin; below them the launches alone"""
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import pace as pace_rule, shape as shape_rule
    chunk, warmup = 16, 8
    gl = torch.Generator().manual_seed(8)
    G, Cn = codec.dmel_groups, codec.decoder.input_channels
    n_steps = warmup + steps
    ids = torch.randint(0, 175, (S, G, chunk * n_steps), generator=gl, dtype=torch.int32).to(dev)
    kw = dict(max_push_tokens=chunk)
    pools = {"no_pace_pool": codec.decode_sessions(S, **kw), "pace_pool_1000": codec.decode_sessions(S, pace=True, **kw),
             "pace_pool_rate": codec.decode_sessions(S, pace=True, **kw)}
    slots = {k: [p.open(**(dict(pace=True) if k != "no_pace_pool" else {})) for _ in range(S)] for k, p in pools.items()}
    for i, s in enumerate(slots["pace_pool_rate"]):
        pools["pace_pool_rate"].set_pace(s, rates[i % len(rates)])
    ms, launches, samples = {k: [] for k in pools}, {k: {} for k in pools}, {k: 0 for k in pools}
    keys, families = list(pools), ("pace", "small")
    for j in range(n_steps):
        noise = [torch.randn(Cn, chunk * 4, device=dev) for _ in range(S)]
        counted = j == n_steps - 1                                          # the launch records of the last step, which is not timed
        for k in (keys if j % 2 == 0 else keys[::-1]):                      # no pool always goes first
            pool = pools[k]
            if counted:
                _lib.prof_reset(); _lib.prof_enable(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.push({s: ids[i, :, j * chunk:(j + 1) * chunk] for i, s in enumerate(slots[k])},
                            noise={s: noise[i] for i, s in enumerate(slots[k])})
            torch.cuda.synchronize()
            if counted:
                launches[k] = {f: _lib.prof_read(f)["launches"] for f in families}
                _lib.prof_enable(False); _lib.prof_reset()
            elif j >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            samples[k] += sum(a.numel() for a, _ in res.values())
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    result, rows = {"sessions": S, "chunk_tokens": chunk, "rates": rates}, []
    for k in keys:
        v = ms[k]
        result[k] = {"median_ms": round(statistics.median(v), 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                     "launches_per_step": launches[k], "audio_samples": samples[k]}
        rows.append(f"{S:8d}  {k:16s}  {statistics.median(v):9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  "
                    f"{launches[k]['pace']:4d}  {launches[k]['small']:5d}  {samples[k]:13d}")
    reports = pools["pace_pool_rate"].paced()
    result["frames"] = {f: sum(getattr(r, f) for r in reports.values()) for f in ("natural", "searched", "quiet")}

    def timed(fn, before=lambda: None):
        v = []
        for j in range(warmup + steps):
            before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if j >= warmup:
                v.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(v), 4), "p10_ms": round(pct(v, 0.1), 4), "p90_ms": round(pct(v, 0.9), 4)}

    # the launches alone: S slots of 16384 new samples, fresh rows every time
    n, vr = 16384, pools[keys[0]].voc_rate
    x = (torch.randn(S, n, device=dev) * 0.3).contiguous()
    alone = {}
    for r in (1000, rates[0]):
        cfg = pace_rule.PaceConfig(initial_permille=r)
        H, D = cfg.samples(vr)
        y = torch.empty(S, pace_rule.max_out(n, H, D), device=dev)
        st = torch.zeros(S, cfg.state_words(vr), dtype=torch.int32, device=dev)
        off, sc = torch.zeros(S, 2 * n // H + 8, dtype=torch.int32, device=dev), torch.zeros(S, 2 * n // H + 8, device=dev)
        tab = torch.empty(pace_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
        w, woff = pace_rule.weight_arena([H], dev)
        alone[f"pace_items_{r}"] = timed(lambda: pace_rule.pace_items([x[s] for s in range(S)], [y[s] for s in range(S)], [cfg] * S, [[]] * S,
                                                                      [pace_rule.FRESH] * S, [False] * S, st, off, sc, vr, w, woff, tab),
                                         st.zero_)
        alone[f"pace_items_{r}"]["searched_frames_per_slot"] = int(st[0, pace_rule.I_SEARCHED])
    scfg = shape_rule.ShapeConfig()
    y = torch.empty(S, n + 2 * shape_rule.MAX_BLOCK, device=dev)
    st = torch.zeros(S, scfg.state_words(vr), dtype=torch.int32, device=dev)
    pk, gn = torch.zeros(S, n // 32 + 2, device=dev), torch.zeros(S, n // 32 + 2, device=dev)
    tab = torch.empty(shape_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    ramps, off = shape_rule.ramp_arena([480], dev)
    alone["shape_items"] = timed(lambda: shape_rule.shape_items([x[s] for s in range(S)], [y[s] for s in range(S)], [scfg] * S,
                                                                [[(0, 1.0, 2.0, 480)]] * S, [1.0] * S, [0] * S, [0] * S, [False] * S, st, pk, gn,
                                                                vr, ramps=ramps, ramp_off=off, table=tab), st.zero_)
    halo = pools[keys[0]].geo.voc_halo
    mel = torch.randn(S, codec.decoder.output_channels, chunk * 4 + 2 * halo, device=dev)
    with torch.no_grad():
        alone["vocoder_call_of_a_step"] = timed(lambda: codec.vocoder(mel))
    result["alone"] = alone
    med = [result[k]["median_ms"] for k in keys]
    searched, voc = alone[f"pace_items_{rates[0]}"]["median_ms"], alone["vocoder_call_of_a_step"]["median_ms"]
    verdict = (f"every slot pacing at 1000 {med[1] - med[0]:+.3f} ms, at {','.join(map(str, rates))} {med[2] - med[0]:+.3f} ms against the pool "
               f"without the option (new work: no threshold); the searched launch alone costs {searched:.4f} ms, "
               + ("MORE than" if searched > voc else "less than") + f" the vocoder call of a step's batch ({voc:.4f} ms)")
    table = [f"{S} decode sessions, {chunk}-token pushes, f32 audio at the vocoder's rate, 100 mel / 10 groups, BigVGAN base "
             f"(tools/bench_stream.py --sessions {S} --pace {','.join(map(str, rates))})",
             f"per-step wall time incl. host synchronisation, {steps} steady-state steps, the three pools interleaved in one process;",
             "no_pace_pool = decode_sessions() as it was; pace_pool_1000 = decode_sessions(pace=True), every slot opened with pace=True at 1000; "
             "pace_pool_rate = the same with set_pace at the rates given",
             "launch records of one step: pace (dmel_pace_items), small (all small kernels, the pace launch among them); samples handed out",
             "sessions  pool              median ms     p10 ms     p90 ms     n  pace  small  audio samples"] + rows + [
             f"frames of pace_pool_rate over the run: {result['frames']}",
             f"launches alone, {S} slots of {n} new samples, fresh rows, wall time incl. host synchronisation (median, p10, p90 ms):"] + [
             f"  {k:24s} {v['median_ms']:9.4f} {v['p10_ms']:9.4f} {v['p90_ms']:9.4f}" +
             (f"   searched frames per slot: {v['searched_frames_per_slot']}" if "searched_frames_per_slot" in v else "")
             for k, v in alone.items()] + [verdict]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


if "--pace" in sys.argv:
    assert "--sessions" in sys.argv, "--pace needs --sessions"
    sessions_pace_section(int(arg_after("--sessions")), [int(r) for r in arg_after("--pace").split(",")], int(arg_after("--steps", "40")),
                          arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "sessions_pace.txt")))
    sys.exit(0)

if "--shape" in sys.argv:
    assert "--sessions" in sys.argv, "--shape needs --sessions"
    sessions_shape_section(int(arg_after("--sessions")), int(arg_after("--output-sample-rate", "0")), arg_after("--sample-format", "f32"),
                           int(arg_after("--steps", "40")),
                           arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                           "sessions_shape.txt")))
    sys.exit(0)

if "--park" in sys.argv:
    assert "--sessions" in sys.argv, "--park needs --sessions"
    sessions_park_section(int(arg_after("--sessions")), int(arg_after("--steps", "40")),
                          arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                          "sessions_park.txt")))
    sys.exit(0)

if "--lookahead" in sys.argv:
    assert "--sessions" in sys.argv, "--lookahead needs --sessions"
    sessions_early_section(int(arg_after("--sessions")), [int(k) for k in arg_after("--lookahead").split(",")],
                           [int(p) for p in arg_after("--push-tokens", "1,4,16").split(",")], int(arg_after("--steps", "40")),
                           arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                           "sessions_early.txt")), arg_after("--label", ""))
    sys.exit(0)

if "--channels" in sys.argv and int(arg_after("--channels")) != 1:
    assert "--sessions" in sys.argv, "--channels needs --sessions"
    wire_format = arg_after("--sample-format", "f32")
    assert wire_format in ("f32", "s16", "ulaw", "alaw"), f"--sample-format {wire_format}: expected f32, s16, ulaw or alaw"
    sessions_channels_section(int(arg_after("--sessions")), [int(r) for r in arg_after("--output-sample-rate", "").split(",") if r],
                              int(arg_after("--steps", "40")),
                              arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                              "sessions_channels.txt")),
                              wire_format, int(arg_after("--channels")))
    sys.exit(0)

if "--sessions" in sys.argv and arg_after("--sample-format", "f32") != "f32":
    wire_format = arg_after("--sample-format")
    assert wire_format in ("s16", "ulaw", "alaw"), f"--sample-format {wire_format}: expected f32, s16, ulaw or alaw"
    sessions_pcm_section(int(arg_after("--sessions")), [int(r) for r in arg_after("--output-sample-rate", "").split(",") if r],
                         int(arg_after("--steps", "40")),
                         arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                         "sessions_pcm.txt" if wire_format == "s16" else "sessions_g711.txt")),
                         wire_format)
    sys.exit(0)

if "--sessions" in sys.argv and "--output-sample-rate" in sys.argv:
    sessions_rates_section(int(arg_after("--sessions")), [int(r) for r in arg_after("--output-sample-rate").split(",")],
                           int(arg_after("--steps", "40")),
                           arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                           "sessions_resample.txt")))
    sys.exit(0)

if "--sessions" in sys.argv:
    sessions_section(int(arg_after("--sessions")),
                     arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                     "decode_sessions_ragged.txt" if "--ragged" in sys.argv else "decode_sessions.txt")),
                     "--ragged" in sys.argv, arg_after("--label", ""))
    sys.exit(0)

if "--output-sample-rate" in sys.argv:
    output_rate_section(int(arg_after("--output-sample-rate")),
                        arg_after("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stream_resample.txt")))
    sys.exit(0)


def pipeline_section():
    # decode_stream(pipeline=True): the vocoder of chunk i on its own stream, overlapping the decoder WaveNet of chunk i + 1 (pieces are
    # yielded one chunk later); 120 s stream, batch 1 and 16, against the sequential generator
    T4L = 2813
    gl = torch.Generator().manual_seed(6)
    ids_long = torch.randint(0, 175, (1, 10, T4L), generator=gl, dtype=torch.int32).to(dev)
    for B in ((1,) if "--batch1" in sys.argv else (1, 16)):
        ids_b = ids_long.expand(B, -1, -1).contiguous()
        for chunk in (32, 64, 128):
            for pipe in (False, True):
                for rep in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = 0
                    for a, m in codec.decode_stream(ids_b, None, chunk_tokens=chunk, pipeline=pipe):
                        n += a.shape[-1]
                    torch.cuda.synchronize()
                    el = time.perf_counter() - t0
                print(json.dumps({"mode": "decode_stream pipeline" if pipe else "decode_stream", "batch": B, "chunk_tokens": chunk,
                                  "audio_s_per_stream": round(n / 24000, 2), "ms_per_chunk": round(el * 1e3 / ((T4L + chunk - 1) // chunk), 3),
                                  "audio_sec_per_sec_all_streams": round(B * n / 24000 / el, 1)}), flush=True)


if ONLY_PIPE:
    pipeline_section()
    sys.exit(0)
for chunk in (8, 32, 64, 128):
    list(codec.decode_stream(ids, flen, chunk_tokens=chunk))      # warm-up (handles, workspaces)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first, first_tokens = None, None
    n = fed = 0
    dec = codec.streaming_decoder(1, flen)
    for a0 in range(0, T4, chunk):
        a, m = dec.push(ids[:, :, a0:a0 + chunk])
        fed = min(T4, a0 + chunk)
        if first is None and a.shape[-1]:
            a.cpu()                               # first audio: include the device->host hand-off
            first, first_tokens = time.perf_counter() - t0, fed
        n += a.shape[-1]
    a, m = dec.finish()
    n += a.shape[-1]
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print(json.dumps({"mode": "state carry", "chunk_tokens": chunk, "first_audio_ms": round(first * 1e3, 2), "first_audio_after_tokens": first_tokens,
                      "audio_s": round(n / 24000, 2), "audio_sec_per_sec": round(n / 24000 / el, 1)}), flush=True)
# the same stream with steady-state pushes replayed as ONE HIP graph each (StreamingDecoder(graph_chunk_tokens=...)), batch 1 and a batch of
# independent streams (what "replicas" of BASELINE config 5 share one GPU as).  A longer stream (120 s) so that the one-time capture and the
# start-up pushes do not dominate; the steady-state time per push is timed separately over the last pushes.
T4L = 2813
gl = torch.Generator().manual_seed(6)
ids_long = torch.randint(0, 175, (1, 10, T4L), generator=gl, dtype=torch.int32).to(dev)
for B in (1, 16):
    ids_b = ids_long.expand(B, -1, -1).contiguous()
    for chunk in (32, 64, 128):
        for graph in (False, True):
            for rep in range(2):                # first pass warms handles / workspaces
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec = codec.streaming_decoder(B, None, True, graph_chunk_tokens=chunk if graph else None)
                n = 0
                starts = list(range(0, T4L, chunk))
                t_steady = None
                for i, a0 in enumerate(starts):
                    if i == len(starts) - 21:
                        torch.cuda.synchronize()
                        t_steady = time.perf_counter()
                    a, m = dec.push(ids_b[:, :, a0:a0 + chunk])
                    n += a.shape[-1]
                    if i == len(starts) - 2:
                        torch.cuda.synchronize()
                        steady_ms = (time.perf_counter() - t_steady) * 1e3 / 20
                a, m = dec.finish()
                n += a.shape[-1]
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
            print(json.dumps({"mode": "state carry + graph replay" if graph else "state carry", "batch": B, "chunk_tokens": chunk,
                              "graph_replays": dec.graph_replays, "pushes": len(starts), "steady_ms_per_push": round(steady_ms, 3),
                              "steady_audio_sec_per_sec_all_streams": round(B * chunk * 4 * 256 / 24000 / (steady_ms * 1e-3), 1),
                              "audio_s_per_stream": round(n / 24000, 2), "audio_sec_per_sec_all_streams": round(B * n / 24000 / el, 1)}), flush=True)
for chunk in (32, 64, 128):
    codec.decode_chunked(ids, flen, chunk_tokens=chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, _ = codec.decode_chunked(ids, flen, chunk_tokens=chunk)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print(json.dumps({"mode": "windows re-run with halo", "chunk_tokens": chunk, "halo_tokens": codec.STREAM_HALO_TOKENS,
                      "audio_sec_per_sec": round(a.shape[-1] / 24000 / el, 1)}), flush=True)
codec.decode(ids, flen, return_audios=True)
torch.cuda.synchronize()
t0 = time.perf_counter()
a, _ = codec.decode(ids, flen, return_audios=True)
torch.cuda.synchronize()
print(json.dumps({"whole_sequence_decode_ms": round((time.perf_counter() - t0) * 1e3, 2), "audio_s": round(a.shape[-1] / 24000, 2)}))
pipeline_section()
