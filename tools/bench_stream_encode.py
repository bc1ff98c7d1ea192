"""Streaming-encode benchmark: per-push time and audio-seconds per second of VQGAN.streaming_encoder for 0.32 s pushes of 24 kHz audio
at batch 1 and batch 16, cfg-2 encoder shapes (80 mel, 8 groups, 70 channels, 20 layers).

    python tools/bench_stream_encode.py [--pushes 62] [--warmup 8] [--out profiles/stream_encode.txt]

The one-launch encoder step and the forced layered step (DMEL_WAVENET_STREAM_FUSED=0, read per call) run INTERLEAVED in one process:
two encoders fed the same audio, push i of one followed by push i of the other, each push bracketed by a host synchronisation and
timed on the wall clock (what a microphone loop pays).  Pushes before the stream's steady state (the first `--warmup`: lookahead fill,
buffer allocation, handle creation) are discarded; medians and the 10th / 90th percentiles are taken over the rest (>= 50).  For
scale, encode() of the whole clip is timed in the same run.  Prints one JSON line and writes the table to --out.

    python tools/bench_stream_encode.py --sample-rate 48000 [--out profiles/stream_resample.txt]

compares, the same way, an encoder fed 0.32 s pushes at the codec's rate (sample_rate=None: no resampler) with one fed 0.32 s pushes of
the same duration at --sample-rate (a StreamResampler in front: two small copies and one resample launch more per push), and APPENDS its
table to --out.

    python tools/bench_stream_encode.py --sessions 16 [--out profiles/stream_sessions.txt]

times a steady-state step of S independent sessions (VQGAN.encode_sessions: one STFT launch and one encoder launch for all of them)
whose starts are offset by a third of a push, so that no two frontiers agree, against what there was for the same job before: S
StreamingEncoder(batch=1) fed the same audio and stepped one after another.  Both run interleaved in one process; a "step" is one push
for every stream, bracketed by a host synchronisation.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --ragged [--label NAME] [--out profiles/encode_sessions_ragged.txt]

the same with the pushes live microphones make: every session pushes its own number of samples in every step, from a seeded list in
[chunk / 2, chunk], so the sessions' feature windows have different lengths in (nearly) every step -- one quantiser call over all of
them in a pool that has quantizer.encode(z, lengths=), one call per group of equal windows in one that has not.  Both --sessions forms
print the quantiser calls per step of the pool.  --label names the table (the commit measured).

    python tools/bench_stream_encode.py --sessions 16 --sample-rate 48000,16000,44100 [--out profiles/sessions_resample.txt]

times a steady-state step of S sessions that arrive at the given rates (slot s at rate s mod len) in a pool that was told the rates
(encode_sessions(sample_rates=...), open(sample_rate=r): ONE resample launch per step, written behind each slot's sample tail) against
what there was for the same job before: the same codec-rate pool behind S StreamResampler(batch=1), one resample launch and two copies
per caller.  Interleaved in one process, equal ids checked, median and 10th / 90th percentile.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --sample-format s16 [--sample-rate 48000,16000] [--out profiles/sessions_pcm.txt]

times a steady-state step of S sessions whose wire carries 16-bit PCM in a pool that was told so (open(sample_format="s16"): ONE convert
launch per step, written where the per-slot copies write) against the same pool with f32 sessions and the conversion every caller
would do in front, `.to(float32) / 32768` per slot.  With --sample-rate the sessions also arrive at those rates (both forms).
Interleaved in one process, equal ids checked, median and 10th / 90th percentile.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --sample-format ulaw|alaw --sample-rate 8000 [--out profiles/sessions_g711.txt]

the same for sessions whose wire carries G.711 (open(sample_format="ulaw" | "alaw"), torch.uint8 codes, telephony's 8 kHz): the
baseline is the same pool with f32 sessions and the expansion every caller would do in front, a 256-entry table gather per slot.

    python tools/bench_stream_encode.py --sessions 16 --channels 2 --sample-format s16 [--sample-rate 48000] [--out profiles/sessions_channels.txt]

times a steady-state step of S sessions whose wire carries interleaved frames of C channels in a pool that was told so
(open(sample_format=..., channels=C): ONE convert launch per step that downmixes on the way) against the same pool with mono f32
sessions and the downmix every caller would do in front, `x.float().sum(1) / C` (with the format's scale or table) per slot.
Interleaved in one process, equal ids asserted, median and 10th / 90th percentile.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --park [--out profiles/sessions_park.txt]

S sessions in steady state, then snapshot + restore of all S of them, as the pool does it -- ONE dmel_stream_pack_items launch per
direction -- against one torch slice .clone() per state tensor per slot and a torch.cat, and the inverse (tools/bench_park.py):
microseconds, bytes moved and GB/s of both, interleaved in one process.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --voice [--label NAME] [--out profiles/sessions_voice.txt]

S staggered sessions with voice detection (a pool built with voice=True, every session opened with voice=True) against the same
sessions in a pool without the option: the same audio (noise with a harmonic burst in every third push), the same pushes, equal ids,
interleaved in one process; then the launches of a step of each pool from the library's profile counters -- what is held is that
the pool without the option launches what it did and the pool with it exactly one kernel more per step that has frames.  Run the
plain --sessions form on the parent commit for the step time before the option existed.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --dtmf [--label NAME] [--out profiles/sessions_dtmf.txt]

The same comparison for DTMF detection (a pool built with dtmf=True, every session opened with dtmf=True; the audio is noise with a
keypad tone pair in every third push): equal ids, and exactly one "dtmf" / one "small" launch record more per step and nothing
else.  No bound on the added time is set; the table shows it next to the plain pool of the same run.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --level [--label NAME] [--out profiles/sessions_level.txt]

Sessions with an input leveller (a pool built with level=True, every session opened with level=True; lines at four levels 6 dB apart,
noise with a tone burst in every third push) against the same sessions in a pool without the option and, for scale, in a pool with
DTMF detection, the three interleaved in one process.  The leveller changes what the encoder sees: the ids of the levelled pool are
checked against encode() of the host rule's output (utils/level.py: scan) for every clip, those of the plain pool against encode();
exactly one "level" / one "small" launch record more per step and nothing else; exit status 1 where a check fails.  Run the plain
--sessions form on the parent commit for the step time before the option existed.  No bound on the added time is set.  APPENDS its
table to --out.

    python tools/bench_stream_encode.py --sessions 16 --echo [--chunk 1920] [--label NAME] [--out profiles/sessions_echo.txt]

Sessions with an echo canceller (a pool built with echo=True, every session opened with echo=True -- 1024 taps, blocks of 32 -- and
pushed its far end with every push; noise through a line of two reflections) against the same sessions in a pool without the option
and, for scale, in a pool with an input leveller, the three interleaved in one process.  The ids and reports of the first two
sessions of the echo pool are checked against encode() / report() of the host rule's output (utils/echo.py: scan; 1024 taps are slow
on the host), those of the plain pool against encode(); exactly one "echo" / one "small" launch record more per step and nothing
else; exit status 1 where a check fails.  The canceller's launch alone (all sessions, one push each) is timed with events as well.
--chunk 1920 makes the pushes 80 ms.  Run the plain --sessions form on the parent commit for the step time before the option
existed.  No bound on the added time is set.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --conceal [--loss 0.05] [--label NAME] [--out profiles/sessions_conceal.txt]

Sessions that conceal lost packets (a pool built with conceal=True, every session opened with conceal=True; voiced-like lines, and
with probability --loss the first 20 ms of a session's push never arrived: push(lost=)) against the same sessions in a pool without
the option, pushed zeros in the place of a loss, and, for scale, in a pool with an input leveller, the three interleaved in one
process.  The ids and reports of the first two sessions of the concealing pool are checked against encode() / report() of the host
rule's output (utils/conceal.py: scan), those of the plain pool against encode() of the zero-filled clips; exactly one "conceal" /
one "small" launch record more per step and nothing else; exit status 1 where a check fails.  The concealment launch alone (all
sessions, one push each, without a loss and with a hole in every slot) is timed with events as well.  Run the plain --sessions form
on the parent commit for the step time before the option existed.  No bound on the added time is set.  APPENDS its table to --out.

    python tools/bench_stream_encode.py --sessions 16 --denoise [--label NAME] [--out profiles/sessions_denoise.txt]

Sessions with a noise suppressor (a pool built with denoise=True, every session opened with denoise=True -- frames of 512, hops of
256; lines with noise floors 6 dB apart and a tone burst in every third push) against the same sessions in a pool without the option
and, for scale, in a pool with an input leveller, the three interleaved in one process.  The ids of every session of the denoising
pool are checked against encode() of the host rule's output (utils/denoise.py: scan), those of the plain pool against encode();
exactly one "denoise" / one "small" launch record more per step and nothing else; exit status 1 where a check fails.  The
suppressor's launch alone (all sessions, one push each) is timed with events as well.  Run the plain --sessions form on the parent
commit for the step time before the option existed.  No bound on the added time is set.  APPENDS its table to --out."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_codec_amd.configs import build_codec

ap = argparse.ArgumentParser()
ap.add_argument("--pushes", type=int, default=62, help="pushes per stream (62 x 0.32 s = 19.84 s)")
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--chunk", type=int, default=7680, help="samples per push (0.32 s at 24 kHz)")
ap.add_argument("--batches", default="1,16")
ap.add_argument("--sample-rate", default=None,
                help="compare pushes at this source rate with pushes at the codec's rate; with --sessions: the sessions' rates, SR[,SR...]")
ap.add_argument("--sessions", type=int, default=0, help="time a step of this many staggered independent sessions")
ap.add_argument("--sample-format", default="f32", choices=("f32", "s16", "ulaw", "alaw"),
                help="with --sessions: s16 / G.711 sessions against torch conversions in front")
ap.add_argument("--channels", type=int, default=1, help="with --sessions: sessions fed interleaved frames of this many channels against the "
                                                        "torch downmix in front")
ap.add_argument("--ragged", action="store_true", help="with --sessions: another push size per session and step (seeded), chunk / 2 .. chunk")
ap.add_argument("--park", action="store_true", help="with --sessions: snapshot + restore of all sessions, one launch against torch slices")
ap.add_argument("--voice", action="store_true", help="with --sessions: sessions with voice detection against the same pool without it")
ap.add_argument("--dtmf", action="store_true", help="with --sessions: sessions with DTMF detection against the same pool without it")
ap.add_argument("--level", action="store_true", help="with --sessions: sessions with an input leveller against the same pool without it")
ap.add_argument("--echo", action="store_true", help="with --sessions: sessions with an echo canceller against the same pool without it")
ap.add_argument("--conceal", action="store_true", help="with --sessions: sessions that conceal lost packets against the same pool without it")
ap.add_argument("--denoise", action="store_true", help="with --sessions: sessions with a noise suppressor against the same pool without it")
ap.add_argument("--loss", type=float, default=0.05, help="with --conceal: the probability that the first 20 ms of a session's push were lost")
ap.add_argument("--label", default="", help="with --sessions: names the table (the commit measured)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
rates = [int(r) for r in args.sample_rate.split(",")] if args.sample_rate else []
args.sample_rate = rates[0] if rates else None
if args.out is None:
    args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                            "sessions_park.txt" if args.sessions and args.park else
                            "sessions_voice.txt" if args.sessions and args.voice else
                            "sessions_level.txt" if args.sessions and args.level else
                            "sessions_echo.txt" if args.sessions and args.echo else
                            "sessions_conceal.txt" if args.sessions and args.conceal else
                            "sessions_denoise.txt" if args.sessions and args.denoise else
                            "sessions_dtmf.txt" if args.sessions and args.dtmf else
                            "sessions_channels.txt" if args.sessions and args.channels > 1 else
                            "sessions_pcm.txt" if args.sessions and args.sample_format == "s16" else
                            "sessions_g711.txt" if args.sessions and args.sample_format != "f32" else
                            "sessions_resample.txt" if args.sessions and rates else "encode_sessions_ragged.txt" if args.sessions and args.ragged else
                            "stream_sessions.txt" if args.sessions else "stream_resample.txt" if args.sample_rate else "stream_encode.txt")
assert args.pushes - args.warmup >= 50, "medians over at least 50 steady-state pushes"
SR = 24000
dev = torch.device("cuda:0")
torch.manual_seed(0)
codec = build_codec(sample_rate=SR, n_mels=80, dmel_groups=8, levels=(7, 5, 5), vocoder=None, decoder_layers=1).to(dev)


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def resample_section():
    """codec-rate pushes against pushes at --sample-rate, interleaved; the source clip is noise at the source rate and the codec-rate
    encoder is fed its resampled form, so both encode the same signal"""
    from dmel_codec_amd.utils.resample import resample
    sr = args.sample_rate
    n_src = args.chunk * sr // SR
    rows, result = [], {"sample_rate": sr, "chunk_s": args.chunk / SR, "pushes": args.pushes, "warmup": args.warmup, "batch": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        src = torch.randn(B, args.pushes * n_src, device=dev) * 0.1
        at_codec = resample(src, sr, SR)[:, :args.pushes * args.chunk].contiguous()
        encs = {"codec_rate": codec.streaming_encoder(B), f"from_{sr}": codec.streaming_encoder(B, sample_rate=sr)}
        feed = {"codec_rate": (at_codec, args.chunk), f"from_{sr}": (src, n_src)}
        ms = {k: [] for k in encs}
        tokens = {k: 0 for k in encs}
        keys = list(encs)
        for i in range(args.pushes):
            for k in (keys if i % 2 == 0 else keys[::-1]):                  # neither path always goes first
                a, n = feed[k]
                t, ids = timed_push(encs[k], a[:, i * n:(i + 1) * n], False)
                tokens[k] += ids.shape[2]
                if i >= args.warmup:
                    ms[k].append(t)
        for e in encs.values():
            e.finish()
        r = {"tokens": tokens}
        for k, v in ms.items():
            med = statistics.median(v)
            r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
            rows.append(f"{B:5d}  {k:11s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
        r["added_median_ms"] = round(r[f"from_{sr}"]["median_ms"] - r["codec_rate"]["median_ms"], 3)
        rows.append(f"{B:5d}  conversion adds {r['added_median_ms']:.3f} ms to the median push ({n_src} source samples -> ~{args.chunk} per item)")
        result["batch"][str(B)] = r
    table = [f"streaming encode from {sr} Hz, 0.32 s pushes, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sample-rate {sr})",
             f"per-push wall time incl. host synchronisation, {args.pushes - args.warmup} steady-state pushes, the two encoders interleaved in one process;",
             "codec_rate = sample_rate=None (no resampler), the other = a StreamResampler in front",
             "batch  input        median ms     p10 ms     p90 ms     n"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(result))


def timed_push(enc, chunk, layered):
    if layered:
        os.environ["DMEL_WAVENET_STREAM_FUSED"] = "0"
    else:
        os.environ.pop("DMEL_WAVENET_STREAM_FUSED", None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = enc.push(chunk)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ids


def sessions_section():
    """S staggered sessions in one pool against S batch-1 encoders stepped in turn; the same audio, the same pushes, equal ids"""
    import random
    S, n = args.sessions, args.chunk
    rng = random.Random(11)
    ragged = [[rng.randint(n // 2, n) for _ in range(S)] for _ in range(args.pushes)]
    audio = torch.randn(S, (args.pushes + 1) * n, device=dev) * 0.1
    pool = codec.encode_sessions(slots=S, max_push_samples=n)
    slots = [pool.open() for _ in range(S)]
    singles = [codec.streaming_encoder(1) for _ in range(S)]
    pos = [0] * S
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    ms = {"sessions": [], "one_by_one": []}
    same, tokens = True, 0
    q_calls, q_encode = [0], codec.quantizer.encode              # quantiser calls of the pool's steps (the counter costs a Python call)

    def counted_encode(*a, **kw):
        q_calls[0] += 1
        return q_encode(*a, **kw)
    calls_per_step = []
    for i in range(args.pushes):
        size = ragged[i] if args.ragged else first if i == 0 else [n] * S
        chunks = [audio[s, pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        got = {}
        for k in (("sessions", "one_by_one") if i % 2 == 0 else ("one_by_one", "sessions")):      # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "sessions":
                codec.quantizer.encode, q_calls[0] = counted_encode, 0
                ids = pool.push({slots[s]: chunks[s] for s in range(S)})
                del codec.quantizer.encode
                got[k] = [ids[slots[s]] for s in range(S)]
            else:
                got[k] = [singles[s].push(chunks[s][None])[0] for s in range(S)]
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
                if k == "sessions":
                    calls_per_step.append(q_calls[0])
        same = same and all(torch.equal(a, b) for a, b in zip(got["sessions"], got["one_by_one"]))
        tokens += sum(a.shape[1] for a in got["sessions"])
    for s in range(S):
        pool.close(slots[s])
        singles[s].finish()
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "ids_equal": bool(same), "tokens": tokens,
         "ragged": args.ragged, "label": args.label,
         "quantizer_calls_per_step": {"mean": round(statistics.mean(calls_per_step), 2), "max": max(calls_per_step)}}
    rows = []
    samples = statistics.mean(sum(v) for v in ragged[args.warmup:]) if args.ragged else S * n      # of a steady-state step, all sessions
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                "audio_s_per_s": round(samples / SR / (med / 1e3), 1)}
        rows.append(f"{S:8d}  {k:10s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {r[k]['audio_s_per_s']:11.1f}  {len(v):4d}")
    r["one_by_one_over_sessions"] = round(r["one_by_one"]["median_ms"] / r["sessions"]["median_ms"], 2)
    rows.append(f"{S:8d}  one pool step is {r['one_by_one_over_sessions']:.2f}x faster than {S} batch-1 pushes in turn; ids equal: {same}")
    rows.append(f"{S:8d}  quantiser calls per pool step: mean {r['quantizer_calls_per_step']['mean']:.2f}, max {r['quantizer_calls_per_step']['max']}")
    pushes = (f"pushes of {n // 2}..{n} samples of 24 kHz audio, another size per session and step (seeded)" if args.ragged else
              "0.32 s pushes of 24 kHz audio, starts staggered by a third of a push")
    table = [(f"[{args.label}] " if args.label else "") + f"independent encode sessions, {pushes}, 80 mel / 8 groups / 70 channels / "
             f"20 layers (tools/bench_stream_encode.py --sessions {S}" + (" --ragged)" if args.ragged else ")"),
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the two "
             "forms interleaved in one process;",
             "sessions = one VQGAN.encode_sessions pool, one_by_one = that many StreamingEncoder(batch=1) stepped in turn",
             "sessions  form        median ms     p10 ms     p90 ms  audio-s / s     n"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))


def sessions_detector_section(opt):
    """S staggered sessions with a detector (opt: "voice" or "dtmf") against the same sessions in a pool without the option; the same
    audio, the same pushes, equal ids; then the launches per step of both pools"""
    import math
    from dmel_codec_amd import _lib
    S, n = args.sessions, args.chunk
    t = torch.arange((args.pushes + 5) * n, device=dev, dtype=torch.float64) / SR
    if opt == "voice":
        tone = (sum(torch.sin(2 * math.pi * 150 * k * t) / k for k in range(1, 21)) * 0.1).float()
    else:                                                                       # the key "5": 770 Hz and 1336 Hz
        tone = ((torch.sin(2 * math.pi * 770 * t) + torch.sin(2 * math.pi * 1336 * t)) * 0.1).float()
    talk = ((torch.arange(t.shape[0], device=dev) // n) % 3 == 0).float()       # a burst in every third push
    audio = torch.randn(S, t.shape[0], device=dev) * 0.01 + tone * talk
    pools = {"plain": codec.encode_sessions(slots=S, max_push_samples=n), opt: codec.encode_sessions(slots=S, max_push_samples=n, **{opt: True})}
    slots = {k: [p.open(**({opt: True} if k == opt else {})) for _ in range(S)] for k, p in pools.items()}
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    pos, ms, same = [0] * S, {k: [] for k in pools}, True

    def step(k, chunks):
        ids = pools[k].push({slots[k][s]: chunks[s] for s in range(S)})
        return [ids[slots[k][s]] for s in range(S)]

    def chunks_of(size):
        nonlocal pos
        c = [audio[s, pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        return c

    for i in range(args.pushes):
        chunks, got = chunks_of(first if i == 0 else [n] * S), {}
        for k in (("plain", opt) if i % 2 == 0 else (opt, "plain")):                  # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[k] = step(k, chunks)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        same = same and all(torch.equal(a, b) for a, b in zip(got["plain"], got[opt]))
    # the launches of a step, from the profile counters (their events cost time: counted behind the timed steps)
    families, launches = ("voice", "dtmf", "small", "stft_logmel", "conv_igemm"), {}
    counted = [chunks_of([n] * S) for _ in range(4)]
    _lib.prof_enable(True)
    for k in pools:
        launches[k] = []
        for chunks in counted:
            _lib.prof_reset()
            step(k, chunks)
            torch.cuda.synchronize()
            launches[k].append({f: _lib.prof_read(f)["launches"] for f in families})
    _lib.prof_enable(False)
    _lib.prof_reset()
    reports = getattr(pools[opt], opt)()
    for k, p in pools.items():
        for s in slots[k]:
            p.close(s)
    held = all(a[opt] == 0 and b[opt] == 1 and b["small"] == a["small"] + 1 and all(b[f] == a[f] for f in families if f not in (opt, "small"))
               for a, b in zip(launches["plain"], launches[opt]))
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "ids_equal": bool(same), "label": args.label,
         "launches_per_step": {k: launches[k][0] for k in pools}, "one_more_launch_per_step": bool(held)}
    if opt == "voice":
        r.update(speech_starts=sorted({rep.starts for rep in reports.values()}), frames=sorted({rep.frames for rep in reports.values()}))
        saw = f"the sessions saw {r['frames']} frames and {r['speech_starts']} speech starts each (a burst in every third push)"
    else:
        r.update(keys=sorted({rep.digits[-4:] for rep in reports.values()}), events=sorted({rep.total for rep in reports.values()}),
                 blocks=sorted({rep.blocks for rep in reports.values()}))
        saw = f"the sessions saw {r['blocks']} blocks and {r['events']} key events each, the last of them {r['keys']} (key 5 in every third push)"
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:6s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  " +
                    "  ".join(f"{f} {launches[k][0][f]}" for f in families))
    r["added_median_ms"] = round(r[opt]["median_ms"] - r["plain"]["median_ms"], 3)
    rows.append(f"{S:8d}  detection adds {r['added_median_ms']:.3f} ms to the median step; ids equal: {same}; the pool without the option "
                f"launches no detector and the pool with it exactly one kernel more per step: {held}")
    rows.append(f"{S:8d}  {saw}")
    table = [(f"[{args.label}] " if args.label else "") + f"encode sessions with {opt} detection, 0.32 s pushes of 24 kHz audio, starts staggered by a "
             f"third of a push, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --{opt})",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the two "
             "pools interleaved in one process;",
             f"plain = encode_sessions(S), {opt} = encode_sessions(S, {opt}=True) with every session opened with {opt}=True; launches: records "
             "of the profile counters in one step",
             "sessions  pool    median ms     p10 ms     p90 ms     n  launches of one step"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))


def sessions_level_section():
    """S staggered sessions with an input leveller against the same sessions in a pool without the option and, for scale, in a pool
    with DTMF detection; the same audio, the same pushes.  The leveller changes what the encoder sees, so its ids are held to the host
    rule: encode() of level.scan of each session's clip; then the launches per step of the pools"""
    import math
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import level as level_rule
    S, n = args.sessions, args.chunk
    t = torch.arange((args.pushes + 5) * n, device=dev, dtype=torch.float64) / SR
    tone = ((torch.sin(2 * math.pi * 770 * t) + torch.sin(2 * math.pi * 1336 * t)) * 0.1).float()
    talk = ((torch.arange(t.shape[0], device=dev) // n) % 3 == 0).float()       # a burst in every third push
    lv = torch.tensor([0.25 * 2 ** (s % 4) for s in range(S)], device=dev)[:, None]        # the lines differ by up to 18 dB
    audio = (torch.randn(S, t.shape[0], device=dev) * 0.01 + tone * talk) * lv
    opts = {"plain": {}, "level": {"level": True}, "dtmf": {"dtmf": True}}
    pools = {k: codec.encode_sessions(slots=S, max_push_samples=n, **o) for k, o in opts.items()}
    slots = {k: [p.open(**opts[k]) for _ in range(S)] for k, p in pools.items()}
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    pos, ms, ids = [0] * S, {k: [] for k in pools}, {k: [[] for _ in range(S)] for k in ("plain", "level")}

    def step(k, chunks):
        out = pools[k].push({slots[k][s]: chunks[s] for s in range(S)})
        return [out[slots[k][s]] for s in range(S)]

    def chunks_of(size):
        nonlocal pos
        c = [audio[s, pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        return c

    order = list(pools)
    for i in range(args.pushes):
        chunks = chunks_of(first if i == 0 else [n] * S)
        for k in order[i % 3:] + order[:i % 3]:                                       # none always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = step(k, chunks)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    # the launches of a step, from the profile counters (their events cost time: counted behind the timed steps)
    families, launches = ("level", "voice", "dtmf", "small", "stft_logmel", "conv_igemm"), {}
    counted = [chunks_of([n] * S) for _ in range(4)]
    _lib.prof_enable(True)
    for k in pools:
        launches[k] = []
        for chunks in counted:
            _lib.prof_reset()
            got = step(k, chunks)
            torch.cuda.synchronize()
            launches[k].append({f: _lib.prof_read(f)["launches"] for f in families})
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    _lib.prof_enable(False)
    _lib.prof_reset()
    reports = pools["level"].levels()
    for k, p in pools.items():
        for s in range(S):
            last = p.close(slots[k][s])
            if k in ids:
                ids[k][s].append(last)
    # the ids: the plain pool's are encode()'s, the levelled pool's encode()'s of the host rule's output
    same = {"plain": True, "level": True}
    for s in range(S):
        x = audio[s, :pos[s]]
        y = level_rule.scan(x.cpu(), level_rule.LevelConfig(), None, SR)[0].to(dev)
        for k, clip in (("plain", x), ("level", y)):
            ref, lens = codec.encode(clip[None], torch.tensor([clip.shape[0]], device=dev))
            same[k] = same[k] and torch.equal(torch.cat(ids[k][s], dim=1), ref[0, :, :int(lens[0])])

    def one_more(opt):
        return all(a[opt] == 0 and b[opt] == 1 and b["small"] == a["small"] + 1 and all(b[f] == a[f] for f in families if f not in (opt, "small"))
                   for a, b in zip(launches["plain"], launches[opt]))
    held = one_more("level") and one_more("dtmf")
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "ids_equal_encode": bool(same["plain"]),
         "ids_equal_encode_of_host_rule": bool(same["level"]), "label": args.label, "launches_per_step": {k: launches[k][0] for k in pools},
         "one_more_launch_per_step": bool(held),
         "gain_db": [round(min(rep.gain_db for rep in reports.values()), 2), round(max(rep.gain_db for rep in reports.values()), 2)],
         "clamped": sorted({rep.clamped for rep in reports.values()}), "blocks": sorted({rep.blocks for rep in reports.values()})}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:6s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  " +
                    "  ".join(f"{f} {launches[k][0][f]}" for f in families))
    r["added_median_ms"] = {k: round(r[k]["median_ms"] - r["plain"]["median_ms"], 3) for k in ("level", "dtmf")}
    rows.append(f"{S:8d}  the leveller adds {r['added_median_ms']['level']:.3f} ms to the median step, the DTMF detector (for scale) "
                f"{r['added_median_ms']['dtmf']:.3f} ms; each pool with an option launches exactly one kernel more per step than the plain one: {held}")
    rows.append(f"{S:8d}  ids of the plain pool equal encode(): {same['plain']}; ids of the levelled pool equal encode() of the host rule's "
                f"output (level.scan of each clip): {same['level']}")
    rows.append(f"{S:8d}  the sessions saw {r['blocks']} blocks each, ended at gains of {r['gain_db'][0]} .. {r['gain_db'][1]} dB and clamped "
                f"{r['clamped']} samples (lines at four levels 6 dB apart, a tone burst in every third push)")
    table = [(f"[{args.label}] " if args.label else "") + "encode sessions with an input leveller, 0.32 s pushes of 24 kHz audio, starts staggered by a "
             f"third of a push, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --level)",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the "
             "three pools interleaved in one process;",
             "plain = encode_sessions(S), level / dtmf = encode_sessions(S, level=True / dtmf=True) with every session opened with the option; "
             "launches: records of the profile counters in one step",
             "sessions  pool    median ms     p10 ms     p90 ms     n  launches of one step"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))
    if not (same["plain"] and same["level"] and held):
        sys.exit(1)


def sessions_echo_section():
    """S staggered sessions with an echo canceller (the defaults: 1024 taps, blocks of 32), each fed its far end with every push,
    against the same sessions in a pool without the option and, for scale, in a pool with an input leveller; the same audio, the
    same pushes.  The canceller changes what the encoder sees, so the ids of its first two sessions are held to the host rule:
    encode() of echo.scan of the session's clip (the host scan of 1024 taps is slow: two sessions, not all); then the launches per
    step of the pools, and the canceller's launch alone -- S slots, one push each -- timed with events"""
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import echo as echo_rule
    S, n = args.sessions, args.chunk
    total = (args.pushes + 5) * n
    far = torch.randn(S, total, device=dev) * 0.05
    mic = torch.zeros_like(far)
    mic[:, 20:] += 0.3 * far[:, :-20]                                         # the line: two reflections and a little noise
    mic[:, 45:] -= 0.15 * far[:, :-45]
    mic += torch.randn(S, total, device=dev) * 0.001
    opts = {"plain": {}, "echo": {"echo": True}, "level": {"level": True}}
    pools = {k: codec.encode_sessions(slots=S, max_push_samples=n, **o) for k, o in opts.items()}
    slots = {k: [p.open(**opts[k]) for _ in range(S)] for k, p in pools.items()}
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    pos, ms, ids = [0] * S, {k: [] for k in pools}, {k: [[] for _ in range(S)] for k in ("plain", "echo")}
    cuts = [[0] for _ in range(S)]

    def step(k, chunks):
        kw = {"far": {slots[k][s]: chunks[s][1] for s in range(S)}} if k == "echo" else {}
        out = pools[k].push({slots[k][s]: chunks[s][0] for s in range(S)}, **kw)
        return [out[slots[k][s]] for s in range(S)]

    def chunks_of(size):
        nonlocal pos
        c = [(mic[s, pos[s]:pos[s] + size[s]], far[s, pos[s]:pos[s] + size[s]]) for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        for s in range(S):
            cuts[s].append(pos[s])
        return c

    order = list(pools)
    for i in range(args.pushes):
        chunks = chunks_of(first if i == 0 else [n] * S)
        for k in order[i % 3:] + order[:i % 3]:                                       # none always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = step(k, chunks)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    # the launches of a step, from the profile counters (their events cost time: counted behind the timed steps)
    families, launches = ("echo", "level", "voice", "dtmf", "small", "stft_logmel", "conv_igemm"), {}
    counted = [chunks_of([n] * S) for _ in range(4)]
    _lib.prof_enable(True)
    for k in pools:
        launches[k] = []
        for chunks in counted:
            _lib.prof_reset()
            got = step(k, chunks)
            torch.cuda.synchronize()
            launches[k].append({f: _lib.prof_read(f)["launches"] for f in families})
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    _lib.prof_enable(False)
    _lib.prof_reset()
    reports = pools["echo"].echoes()
    for k, p in pools.items():
        for s in range(S):
            last = p.close(slots[k][s])
            if k in ids:
                ids[k][s].append(last)
    # the ids: the plain pool's are encode()'s, the echo pool's encode()'s of the host rule's output, push by push
    same, checked = {"plain": True, "echo": True}, min(S, 2)
    for s in range(S):
        x = mic[s, :pos[s]]
        clips = [("plain", x)]
        if s < checked:
            xs, fs, state, out = x.cpu(), far[s, :pos[s]].cpu(), None, []
            for a, b in zip(cuts[s], cuts[s][1:]):
                e, state, _, _ = echo_rule.scan(xs[a:b], fs[a:b], echo_rule.EchoConfig(), state)
                out.append(e)
            clips.append(("echo", torch.cat(out).to(dev)))
            same["echo"] = same["echo"] and reports[slots["echo"][s]] == echo_rule.report(state)
        for k, clip in clips:
            ref, lens = codec.encode(clip[None], torch.tensor([clip.shape[0]], device=dev))
            same[k] = same[k] and torch.equal(torch.cat(ids[k][s], dim=1), ref[0, :, :int(lens[0])])

    def one_more(opt):
        return all(a[opt] == 0 and b[opt] == 1 and b["small"] == a["small"] + 1 and all(b[f] == a[f] for f in families if f not in (opt, "small"))
                   for a, b in zip(launches["plain"], launches[opt]))
    held = one_more("echo") and one_more("level")
    # the canceller's launch alone: S slots that gain one push each, the far end with it, timed with events
    cfg = echo_rule.EchoConfig()
    rows_ = mic[:, :n].contiguous()
    state = torch.zeros(S, echo_rule.ROW_WORDS, dtype=torch.int32, device=dev)
    pitch = echo_rule.max_blocks(n, cfg.block_samples) + 1
    o1, o2 = torch.zeros(S, pitch, device=dev), torch.zeros(S, pitch, device=dev)
    tab = torch.empty(echo_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    alone = []
    for i in range(args.pushes):
        a = i * n
        rows_.copy_(mic[:, a:a + n])
        fars = [far[s, a:a + n].contiguous() for s in range(S)]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        echo_rule.echo_items(rows_, [0] * S, [n] * S, fars, [cfg] * S, state, o1, o2, table=tab)
        ev1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            alone.append(ev0.elapsed_time(ev1))
    erle = sorted(rep.erle_db for rep in reports.values())
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "ids_equal_encode": bool(same["plain"]),
         "ids_equal_encode_of_host_rule": bool(same["echo"]), "sessions_checked_against_host_rule": checked, "label": args.label,
         "launches_per_step": {k: launches[k][0] for k in pools}, "one_more_launch_per_step": bool(held),
         "erle_db": [round(erle[0], 1), round(erle[-1], 1)], "taps": cfg.taps, "block_samples": cfg.block_samples,
         "echo_launch_alone_ms": {"median": round(statistics.median(alone), 4), "p10": round(pct(alone, 0.1), 4),
                                  "p90": round(pct(alone, 0.9), 4), "n": len(alone)}}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:6s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  " +
                    "  ".join(f"{f} {launches[k][0][f]}" for f in families))
    r["added_median_ms"] = {k: round(r[k]["median_ms"] - r["plain"]["median_ms"], 3) for k in ("echo", "level")}
    rows.append(f"{S:8d}  the canceller adds {r['added_median_ms']['echo']:.3f} ms to the median step, the leveller (for scale) "
                f"{r['added_median_ms']['level']:.3f} ms; each pool with an option launches exactly one kernel more per step than the plain one: {held}")
    rows.append(f"{S:8d}  the canceller's launch alone ({S} slots x {n} samples, {cfg.taps} taps, blocks of {cfg.block_samples}; events around "
                f"echo_items, its table launch included): median {r['echo_launch_alone_ms']['median']:.4f} ms, p10 "
                f"{r['echo_launch_alone_ms']['p10']:.4f}, p90 {r['echo_launch_alone_ms']['p90']:.4f} over {len(alone)} launches")
    rows.append(f"{S:8d}  ids of the plain pool equal encode(): {same['plain']}; ids and reports of the first {checked} sessions of the echo pool "
                f"equal encode() / report() of the host rule (echo.scan of each clip): {same['echo']}")
    rows.append(f"{S:8d}  the sessions ended at a metered ERLE of {r['erle_db'][0]} .. {r['erle_db'][1]} dB (noise far end, a line of two reflections)")
    table = [(f"[{args.label}] " if args.label else "") + f"encode sessions with an echo canceller, {n / SR:.2f} s pushes of 24 kHz audio, starts "
             f"staggered by a third of a push, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --echo"
             + (f" --chunk {n}" if n != 7680 else "") + ")",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the "
             "three pools interleaved in one process;",
             "plain = encode_sessions(S), echo / level = encode_sessions(S, echo=True / level=True) with every session opened with the option; "
             "launches: records of the profile counters in one step",
             "sessions  pool    median ms     p10 ms     p90 ms     n  launches of one step"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))
    if not (same["plain"] and same["echo"] and held):
        sys.exit(1)


def sessions_conceal_section():
    """S staggered sessions that conceal lost packets against the same sessions in a pool without the option, which are pushed zeros
    in the place of a loss, and, for scale, in a pool with an input leveller (the comparable one-workgroup-per-slot launch); the same
    audio, the same pushes, the same losses: with probability --loss the first 20 ms of a session's push never arrived.  The option
    changes what the encoder sees, so the ids of the first two sessions are held to the host rule: encode() of conceal.scan of the
    zero-filled clip; then the launches per step of the pools, and the concealment launch alone -- S slots, one push each, without a
    loss and with one in every slot -- timed with events"""
    import math, random
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import conceal as conceal_rule
    S, n, hole = args.sessions, args.chunk, 480
    rng = random.Random(13)
    total = (args.pushes + 5) * n
    t = torch.arange(total, device=dev, dtype=torch.float64) / SR
    f0 = [90.0 + 17.0 * s for s in range(S)]                                   # a voiced-like line per session: eight harmonics and noise
    audio = torch.stack([sum(torch.sin(2 * math.pi * f * h * t) * (0.2 / h) for h in range(1, 9)).float() for f in f0])
    audio += torch.randn(S, total, device=dev) * 0.003
    opts = {"plain": {}, "conceal": {"conceal": True}, "level": {"level": True}}
    pools = {k: codec.encode_sessions(slots=S, max_push_samples=n, **o) for k, o in opts.items()}
    slots = {k: [p.open(**opts[k]) for _ in range(S)] for k, p in pools.items()}
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    pos, ms, ids = [0] * S, {k: [] for k in pools}, {k: [[] for _ in range(S)] for k in ("plain", "conceal")}
    ranges, n_lost = [[] for _ in range(S)], 0

    def step(k, chunks):
        if k == "conceal":
            out = pools[k].push({slots[k][s]: c[hole:] if gone else c for s, (c, gone) in enumerate(chunks)},
                                lost={slots[k][s]: hole for s, (c, gone) in enumerate(chunks) if gone})
        else:
            out = pools[k].push({slots[k][s]: c for s, (c, gone) in enumerate(chunks)})
        return [out[slots[k][s]] for s in range(S)]

    def chunks_of(size):
        nonlocal pos, n_lost
        c = []
        for s in range(S):
            gone = size[s] > hole and rng.random() < args.loss
            if gone:                                                           # what a caller without the option pushes: zeros
                audio[s, pos[s]:pos[s] + hole] = 0.0
                ranges[s].append((pos[s], pos[s] + hole))
                n_lost += 1
            c.append((audio[s, pos[s]:pos[s] + size[s]], gone))
        pos = [p + k for p, k in zip(pos, size)]
        return c

    order = list(pools)
    for i in range(args.pushes):
        chunks = chunks_of(first if i == 0 else [n] * S)
        for k in order[i % 3:] + order[:i % 3]:                                       # none always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = step(k, chunks)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    # the launches of a step, from the profile counters (their events cost time: counted behind the timed steps)
    families, launches = ("conceal", "level", "voice", "dtmf", "small", "stft_logmel", "conv_igemm"), {}
    saved, args.loss = args.loss, 0.0                                          # the counted steps lose nothing: the same work in every pool
    counted = [chunks_of([n] * S) for _ in range(4)]
    args.loss = saved
    _lib.prof_enable(True)
    for k in pools:
        launches[k] = []
        for chunks in counted:
            _lib.prof_reset()
            got = step(k, chunks)
            torch.cuda.synchronize()
            launches[k].append({f: _lib.prof_read(f)["launches"] for f in families})
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    _lib.prof_enable(False)
    _lib.prof_reset()
    reports = pools["conceal"].concealed()
    for k, p in pools.items():
        for s in range(S):
            last = p.close(slots[k][s])
            if k in ids:
                ids[k][s].append(last)
    # the ids: the plain pool's are encode()'s of the zero-filled clip, the concealing pool's encode()'s of the host rule's output
    same, checked = {"plain": True, "conceal": True}, min(S, 2)
    for s in range(S):
        x = audio[s, :pos[s]]
        clips = [("plain", x)]
        if s < checked:
            xs, state, out, at = x.cpu(), None, [], 0
            for lo, hi in ranges[s] + [(pos[s], pos[s])]:                       # one call per range: a call takes at most 16
                y, state, _, _ = conceal_rule.scan(xs[at:hi], [(lo - at, hi - at)] if hi > lo else [], conceal_rule.ConcealConfig(), state, SR)
                out.append(y)
                at = hi
            clips.append(("conceal", torch.cat(out).to(dev)))
            same["conceal"] = same["conceal"] and reports[slots["conceal"][s]] == conceal_rule.report(state, SR)
        for k, clip in clips:
            ref, lens = codec.encode(clip[None], torch.tensor([clip.shape[0]], device=dev))
            same[k] = same[k] and torch.equal(torch.cat(ids[k][s], dim=1), ref[0, :, :int(lens[0])])

    def one_more(opt):
        return all(a[opt] == 0 and b[opt] == 1 and b["small"] == a["small"] + 1 and all(b[f] == a[f] for f in families if f not in (opt, "small"))
                   for a, b in zip(launches["plain"], launches[opt]))
    held = one_more("conceal") and one_more("level")
    # the concealment launch alone: S slots that gain one push each, timed with events; without a loss, then with one in every slot
    cfg = conceal_rule.ConcealConfig()
    rows_ = audio[:, :n].contiguous()
    state = torch.zeros(S, conceal_rule.ROW_WORDS, dtype=torch.int32, device=dev)
    o1 = torch.zeros(S, conceal_rule.MAX_RANGES, dtype=torch.int32, device=dev)
    o2 = torch.zeros(S, conceal_rule.MAX_RANGES, device=dev)
    tab = torch.empty(conceal_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    alone = {"no_loss": [], "every_slot": []}
    for i in range(2 * args.pushes):
        a, which = (i // 2) * n, "every_slot" if i % 2 else "no_loss"
        rows_.copy_(audio[:, a:a + n])
        rg = [[(n // 2, n // 2 + hole)] if i % 2 and n > 2 * hole else [] for _ in range(S)]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        conceal_rule.conceal_items(rows_, [0] * S, [n] * S, rg, [cfg] * S, state, o1, o2, sample_rate=SR, table=tab)
        ev1.record()
        torch.cuda.synchronize()
        if i >= 2 * args.warmup:
            alone[which].append(ev0.elapsed_time(ev1))
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "loss": args.loss, "lost_packets": n_lost,
         "ids_equal_encode": bool(same["plain"]), "ids_equal_encode_of_host_rule": bool(same["conceal"]),
         "sessions_checked_against_host_rule": checked, "label": args.label, "launches_per_step": {k: launches[k][0] for k in pools},
         "one_more_launch_per_step": bool(held),
         "lost_samples": sorted({rep.lost_samples for rep in reports.values()}), "muted_samples": sorted({rep.muted_samples for rep in reports.values()}),
         "conceal_launch_alone_ms": {k: {"median": round(statistics.median(v), 4), "p10": round(pct(v, 0.1), 4), "p90": round(pct(v, 0.9), 4),
                                         "n": len(v)} for k, v in alone.items()}}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:7s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  " +
                    "  ".join(f"{f} {launches[k][0][f]}" for f in families))
    r["added_median_ms"] = {k: round(r[k]["median_ms"] - r["plain"]["median_ms"], 3) for k in ("conceal", "level")}
    rows.append(f"{S:8d}  concealment adds {r['added_median_ms']['conceal']:.3f} ms to the median step, the leveller (for scale) "
                f"{r['added_median_ms']['level']:.3f} ms; each pool with an option launches exactly one kernel more per step than the plain one: {held}")
    la = r["conceal_launch_alone_ms"]
    rows.append(f"{S:8d}  the concealment launch alone ({S} slots x {n} samples; events around conceal_items, its table launch included): "
                f"median {la['no_loss']['median']:.4f} ms (p10 {la['no_loss']['p10']:.4f}, p90 {la['no_loss']['p90']:.4f}) without a loss, "
                f"{la['every_slot']['median']:.4f} ms (p10 {la['every_slot']['p10']:.4f}, p90 {la['every_slot']['p90']:.4f}) with a 20 ms hole, "
                f"a search of 301 lags, in every slot; {len(alone['no_loss'])} launches each")
    rows.append(f"{S:8d}  ids of the plain pool equal encode() of the zero-filled clips: {same['plain']}; ids and reports of the first {checked} "
                f"sessions of the concealing pool equal encode() / report() of the host rule (conceal.scan of each clip): {same['conceal']}")
    rows.append(f"{S:8d}  {n_lost} packets of 20 ms were lost (--loss {args.loss}); the sessions ended with {r['lost_samples']} lost and "
                f"{r['muted_samples']} muted samples")
    table = [(f"[{args.label}] " if args.label else "") + f"encode sessions that conceal lost packets, {n / SR:.2f} s pushes of 24 kHz audio, starts "
             f"staggered by a third of a push, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --conceal "
             f"--loss {args.loss}" + (f" --chunk {n}" if n != 7680 else "") + ")",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the "
             "three pools interleaved in one process;",
             "plain = encode_sessions(S), conceal / level = encode_sessions(S, conceal=True / level=True) with every session opened with the "
             "option; launches: records of the profile counters in one step",
             "sessions  pool     median ms     p10 ms     p90 ms     n  launches of one step"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))
    if not (same["plain"] and same["conceal"] and held):
        sys.exit(1)


def sessions_denoise_section():
    """S staggered sessions with a noise suppressor against the same sessions in a pool without the option and, for scale, in a pool
    with an input leveller (the comparable one-workgroup-per-slot launch); the same audio, the same pushes.  The suppressor changes
    what the encoder sees, so its ids are held to the host rule: encode() of denoise.scan of each session's clip; then the launches
    per step of the pools, and the suppressor's launch alone -- S slots, one push each -- timed with events"""
    import math
    from dmel_codec_amd import _lib
    from dmel_codec_amd.utils import denoise as denoise_rule
    S, n = args.sessions, args.chunk
    t = torch.arange((args.pushes + 5) * n, device=dev, dtype=torch.float64) / SR
    tone = ((torch.sin(2 * math.pi * 770 * t) + torch.sin(2 * math.pi * 1336 * t)) * 0.1).float()
    talk = ((torch.arange(t.shape[0], device=dev) // n) % 3 == 0).float()       # a burst in every third push
    lv = torch.tensor([0.0025 * 2 ** (s % 4) for s in range(S)], device=dev)[:, None]      # noise floors of -52 .. -34 dBFS
    audio = torch.randn(S, t.shape[0], device=dev) * lv + tone * talk
    opts = {"plain": {}, "denoise": {"denoise": True}, "level": {"level": True}}
    pools = {k: codec.encode_sessions(slots=S, max_push_samples=n, **o) for k, o in opts.items()}
    slots = {k: [p.open(**opts[k]) for _ in range(S)] for k, p in pools.items()}
    first = [n * (1 + s % 3) // 3 for s in range(S)]            # the starts differ by a third of a push
    pos, ms, ids = [0] * S, {k: [] for k in pools}, {k: [[] for _ in range(S)] for k in ("plain", "denoise")}

    def step(k, chunks):
        out = pools[k].push({slots[k][s]: chunks[s] for s in range(S)})
        return [out[slots[k][s]] for s in range(S)]

    def chunks_of(size):
        nonlocal pos
        c = [audio[s, pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        return c

    order = list(pools)
    for i in range(args.pushes):
        chunks = chunks_of(first if i == 0 else [n] * S)
        for k in order[i % 3:] + order[:i % 3]:                                       # none always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = step(k, chunks)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    # the launches of a step, from the profile counters (their events cost time: counted behind the timed steps)
    families, launches = ("denoise", "level", "voice", "dtmf", "small", "stft_logmel", "conv_igemm"), {}
    counted = [chunks_of([n] * S) for _ in range(4)]
    _lib.prof_enable(True)
    for k in pools:
        launches[k] = []
        for chunks in counted:
            _lib.prof_reset()
            got = step(k, chunks)
            torch.cuda.synchronize()
            launches[k].append({f: _lib.prof_read(f)["launches"] for f in families})
            if k in ids:
                for s in range(S):
                    ids[k][s].append(got[s])
    _lib.prof_enable(False)
    _lib.prof_reset()
    reports = pools["denoise"].denoised()
    for k, p in pools.items():
        for s in range(S):
            last = p.close(slots[k][s])
            if k in ids:
                ids[k][s].append(last)
    # the ids: the plain pool's are encode()'s, the denoising pool's encode()'s of the host rule's output; the reports the host's
    same, cfg = {"plain": True, "denoise": True}, denoise_rule.DenoiseConfig()
    for s in range(S):
        x = audio[s, :pos[s]]
        y, state, _, _ = denoise_rule.scan(x.cpu(), cfg)
        same["denoise"] = same["denoise"] and reports[slots["denoise"][s]] == denoise_rule.report(state, cfg.frame_samples, SR, cfg.learn_frames)
        for k, clip in (("plain", x), ("denoise", y.to(dev))):
            ref, lens = codec.encode(clip[None], torch.tensor([clip.shape[0]], device=dev))
            same[k] = same[k] and torch.equal(torch.cat(ids[k][s], dim=1), ref[0, :, :int(lens[0])])

    def one_more(opt):
        return all(a[opt] == 0 and b[opt] == 1 and b["small"] == a["small"] + 1 and all(b[f] == a[f] for f in families if f not in (opt, "small"))
                   for a, b in zip(launches["plain"], launches[opt]))
    held = one_more("denoise") and one_more("level")
    # the suppressor's launch alone: S slots that gain one push each, timed with events
    rows_ = audio[:, :n].contiguous()
    state = torch.zeros(S, denoise_rule.STATE_WORDS, dtype=torch.int32, device=dev)
    pitch = denoise_rule.max_frames(n, cfg.frame_samples) + 1
    o1, o2 = torch.zeros(S, pitch, device=dev), torch.zeros(S, pitch, device=dev)
    tab = torch.empty(denoise_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    transform = denoise_rule.transform_table().to(dev)
    alone = []
    for i in range(args.pushes):
        a = i * n
        rows_.copy_(audio[:, a:a + n])
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        denoise_rule.denoise_items(rows_, [0] * S, [n] * S, [cfg] * S, state, o1, o2, transform, table=tab)
        ev1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            alone.append(ev0.elapsed_time(ev1))
    att = sorted(rep.attenuation_db for rep in reports.values())
    r = {"sessions": S, "chunk_s": n / SR, "pushes": args.pushes, "warmup": args.warmup, "ids_equal_encode": bool(same["plain"]),
         "ids_and_reports_equal_host_rule": bool(same["denoise"]), "label": args.label,
         "launches_per_step": {k: launches[k][0] for k in pools}, "one_more_launch_per_step": bool(held),
         "attenuation_db": [round(att[0], 2), round(att[-1], 2)], "frames": sorted({rep.frames for rep in reports.values()}),
         "frame_samples": cfg.frame_samples,
         "denoise_launch_alone_ms": {"median": round(statistics.median(alone), 4), "p10": round(pct(alone, 0.1), 4),
                                     "p90": round(pct(alone, 0.9), 4), "n": len(alone)}}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:7s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}  " +
                    "  ".join(f"{f} {launches[k][0][f]}" for f in families))
    r["added_median_ms"] = {k: round(r[k]["median_ms"] - r["plain"]["median_ms"], 3) for k in ("denoise", "level")}
    rows.append(f"{S:8d}  the suppressor adds {r['added_median_ms']['denoise']:.3f} ms to the median step, the leveller (for scale) "
                f"{r['added_median_ms']['level']:.3f} ms; each pool with an option launches exactly one kernel more per step than the plain one: {held}")
    rows.append(f"{S:8d}  the suppressor's launch alone ({S} slots x {n} samples, frames of {cfg.frame_samples}: {n // cfg.hop} frames per slot; events "
                f"around denoise_items, its table launch included): median {r['denoise_launch_alone_ms']['median']:.4f} ms, p10 "
                f"{r['denoise_launch_alone_ms']['p10']:.4f}, p90 {r['denoise_launch_alone_ms']['p90']:.4f} over {len(alone)} launches")
    rows.append(f"{S:8d}  ids of the plain pool equal encode(): {same['plain']}; ids and reports of the denoising pool equal encode() / report() "
                f"of the host rule (denoise.scan of each clip): {same['denoise']}")
    rows.append(f"{S:8d}  the sessions saw {r['frames']} frames each and attenuated their streams by {r['attenuation_db'][0]} .. "
                f"{r['attenuation_db'][1]} dB, the tone bursts included (noise floors 6 dB apart, a tone burst in every third push)")
    table = [(f"[{args.label}] " if args.label else "") + "encode sessions with a noise suppressor, 0.32 s pushes of 24 kHz audio, starts staggered by a "
             f"third of a push, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --denoise)",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the "
             "three pools interleaved in one process;",
             "plain = encode_sessions(S), denoise / level = encode_sessions(S, denoise=True / level=True) with every session opened with the "
             "option; launches: records of the profile counters in one step",
             "sessions  pool     median ms     p10 ms     p90 ms     n  launches of one step"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))
    if not (same["plain"] and same["denoise"] and held):
        sys.exit(1)


def sessions_resample_section():
    """S staggered sessions at their own rates: one pool that converts them in one launch against the codec-rate pool behind S
    StreamResampler(batch=1); the same audio, the same pushes, equal ids"""
    from dmel_codec_amd.models.stream_schedule import resample_max_outputs
    from dmel_codec_amd.utils.resample import StreamResampler
    S = args.sessions
    rate = [rates[s % len(rates)] for s in range(S)]
    n = [args.chunk * r // SR for r in rate]                     # 0.32 s of every slot's own rate
    audio = [torch.randn((args.pushes + 1) * n[s], device=dev) * 0.1 for s in range(S)]
    pool = codec.encode_sessions(slots=S, max_push_samples=max(n), sample_rates=rates)
    slots = [pool.open(sample_rate=rate[s]) for s in range(S)]
    behind = codec.encode_sessions(slots=S, max_push_samples=max(resample_max_outputs(r, SR, max(n)) for r in rates))
    bslots = [behind.open() for _ in range(S)]
    front = [StreamResampler(rate[s], SR, 1) for s in range(S)]
    pos = [0] * S
    first = [n[s] * (1 + s % 3) // 3 for s in range(S)]          # the starts differ by a third of a push
    ms = {"per_slot_rates": [], "resamplers_in_front": []}
    same, tokens = True, 0
    for i in range(args.pushes):
        size = first if i == 0 else n
        chunks = [audio[s][pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        got = {}
        keys = list(ms)
        for k in (keys if i % 2 == 0 else keys[::-1]):           # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "per_slot_rates":
                ids = pool.push({slots[s]: chunks[s] for s in range(S)})
                got[k] = [ids[slots[s]] for s in range(S)]
            else:
                ids = behind.push({bslots[s]: front[s].push(chunks[s][None])[0] for s in range(S)})
                got[k] = [ids[bslots[s]] for s in range(S)]
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        same = same and all(torch.equal(a, b) for a, b in zip(*got.values()))
        tokens += sum(a.shape[1] for a in got["per_slot_rates"])
    r = {"sessions": S, "sample_rates": rates, "chunk_s": args.chunk / SR, "pushes": args.pushes, "warmup": args.warmup,
         "ids_equal": bool(same), "tokens": tokens}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:19s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    r["in_front_over_per_slot"] = round(r["resamplers_in_front"]["median_ms"] / r["per_slot_rates"]["median_ms"], 3)
    rows.append(f"{S:8d}  median step with {S} resamplers in front / with per-slot rates: {r['in_front_over_per_slot']:.3f}; ids equal: {same}")
    table = [f"encode sessions at {','.join(map(str, rates))} Hz, 0.32 s pushes, starts staggered by a third of a push, 80 mel / 8 groups / "
             f"70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --sample-rate {','.join(map(str, rates))})",
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the two "
             "forms interleaved in one process;",
             "per_slot_rates = encode_sessions(sample_rates=...): one resample launch per step; resamplers_in_front = the codec-rate pool behind "
             "one StreamResampler(batch=1) per session",
             "sessions  form                 median ms     p10 ms     p90 ms     n"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))


def sessions_pcm_section():
    """S staggered s16 or G.711 sessions (at their own rates, if any were given): one pool that converts all slots in one launch
    against the same pool with f32 sessions behind one torch conversion per slot (s16: a cast and a scale; G.711: a 256-entry table
    gather); the same samples, the same pushes, equal ids"""
    from dmel_codec_amd.utils import pcm
    S, fmt = args.sessions, args.sample_format
    wire = f"{fmt}_sessions"
    rate = [rates[s % len(rates)] if rates else SR for s in range(S)]
    n = [args.chunk * r // SR for r in rate]                     # 0.32 s of every slot's own rate
    noise = [torch.randn((args.pushes + 1) * n[s], device=dev) * 0.1 for s in range(S)]
    if fmt == "s16":
        audio = [(x * 32768).round().clamp(-32768, 32767).to(torch.int16) for x in noise]
        in_front = lambda c: c.to(torch.float32) / 32768
    else:
        audio = [pcm.to_g711(x, fmt) for x in noise]
        lut = pcm.from_g711(torch.arange(256, device=dev).to(torch.uint8), fmt)         # what a caller keeps: code -> float
        in_front = lambda c: lut[c.long()]
    pools = {wire: codec.encode_sessions(slots=S, max_push_samples=max(n), sample_rates=rates),
             "torch_in_front": codec.encode_sessions(slots=S, max_push_samples=max(n), sample_rates=rates)}
    slots = {wire: [pools[wire].open(sample_rate=rate[s], sample_format=fmt) for s in range(S)],
             "torch_in_front": [pools["torch_in_front"].open(sample_rate=rate[s]) for s in range(S)]}
    pos = [0] * S
    first = [n[s] * (1 + s % 3) // 3 for s in range(S)]          # the starts differ by a third of a push
    ms = {k: [] for k in pools}
    same, tokens = True, 0
    for i in range(args.pushes):
        size = first if i == 0 else n
        chunks = [audio[s][pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        got = {}
        keys = list(ms)
        for k in (keys if i % 2 == 0 else keys[::-1]):           # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == wire:
                ids = pools[k].push({slots[k][s]: chunks[s] for s in range(S)})
            else:
                ids = pools[k].push({slots[k][s]: in_front(chunks[s]) for s in range(S)})
            got[k] = [ids[slots[k][s]] for s in range(S)]
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        same = same and all(torch.equal(a, b) for a, b in zip(*got.values()))
        tokens += sum(a.shape[1] for a in got[wire])
    r = {"sessions": S, "sample_format": fmt, "sample_rates": rates or [SR], "chunk_s": args.chunk / SR, "pushes": args.pushes,
         "warmup": args.warmup, "ids_equal": bool(same), "tokens": tokens}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:14s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    r[f"torch_over_{fmt}"] = round(r["torch_in_front"]["median_ms"] / r[wire]["median_ms"], 3)
    rows.append(f"{S:8d}  median step with {S} torch conversions in front / with {fmt} sessions: {r[f'torch_over_{fmt}']:.3f}; ids equal: {same}")
    what = ",".join(map(str, rates)) if rates else "the codec's rate"
    name = {"s16": "16-bit PCM", "ulaw": "G.711 mu-law", "alaw": "G.711 A-law"}[fmt]
    table = [f"encode sessions fed {name} at {what}, 0.32 s pushes, starts staggered by a third of a push, 80 mel / 8 groups / 70 channels / "
             f"20 layers (tools/bench_stream_encode.py --sessions {S} --sample-format {fmt}" + (f" --sample-rate {what})" if rates else ")"),
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the two "
             "forms interleaved in one process;",
             f"{wire} = open(sample_format=\"{fmt}\"): one convert launch per step; torch_in_front = f32 sessions, " +
             (".to(float32) / 32768 per slot" if fmt == "s16" else "a 256-entry table gather per slot"),
             "sessions  form            median ms     p10 ms     p90 ms     n"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))


def sessions_channels_section():
    """S staggered sessions fed interleaved frames of C channels in the chosen format (at their own rates, if any were given): one
    pool that downmixes all slots in its one convert launch against the same pool with mono f32 sessions behind one torch downmix per
    slot; the same frames, the same pushes, equal ids"""
    from dmel_codec_amd.utils import pcm
    S, fmt, ch = args.sessions, args.sample_format, args.channels
    wire = f"{ch}ch_sessions"
    rate = [rates[s % len(rates)] if rates else SR for s in range(S)]
    n = [args.chunk * r // SR for r in rate]                     # 0.32 s of every slot's own rate, in frames
    noise = [torch.randn((args.pushes + 1) * n[s], ch, device=dev) * 0.1 for s in range(S)]
    # the divisor lives on the device: torch divides by a Python scalar as a multiply by its rounded reciprocal, which is not the rule
    div = torch.full((), float(ch) * (32768.0 if fmt == "s16" else 1.0), device=dev)
    if fmt == "f32":
        audio = noise
        in_front = lambda c: c.sum(1) / div
    elif fmt == "s16":
        audio = [(x * 32768).round().clamp(-32768, 32767).to(torch.int16) for x in noise]
        in_front = lambda c: c.to(torch.float32).sum(1) / div   # the sum of up to 8 s16 values is exact in fp32
    else:
        audio = [pcm.to_g711(x.reshape(-1), fmt).view(-1, ch) for x in noise]
        lut = pcm.from_g711(torch.arange(256, device=dev).to(torch.uint8), fmt)         # what a caller keeps: code -> float
        in_front = lambda c: lut[c.long()].sum(1) / div
    pools = {wire: codec.encode_sessions(slots=S, max_push_samples=max(n), sample_rates=rates),
             "torch_in_front": codec.encode_sessions(slots=S, max_push_samples=max(n), sample_rates=rates)}
    slots = {wire: [pools[wire].open(sample_rate=rate[s], sample_format=fmt, channels=ch) for s in range(S)],
             "torch_in_front": [pools["torch_in_front"].open(sample_rate=rate[s]) for s in range(S)]}
    pos = [0] * S
    first = [n[s] * (1 + s % 3) // 3 for s in range(S)]          # the starts differ by a third of a push
    ms = {k: [] for k in pools}
    same, tokens = True, 0
    for i in range(args.pushes):
        size = first if i == 0 else n
        chunks = [audio[s][pos[s]:pos[s] + size[s]] for s in range(S)]
        pos = [p + k for p, k in zip(pos, size)]
        got = {}
        keys = list(ms)
        for k in (keys if i % 2 == 0 else keys[::-1]):           # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == wire:
                ids = pools[k].push({slots[k][s]: chunks[s] for s in range(S)})
            else:
                ids = pools[k].push({slots[k][s]: in_front(chunks[s]) for s in range(S)})
            got[k] = [ids[slots[k][s]] for s in range(S)]
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        same = same and all(torch.equal(a, b) for a, b in zip(*got.values()))
        tokens += sum(a.shape[1] for a in got[wire])
    r = {"sessions": S, "channels": ch, "sample_format": fmt, "sample_rates": rates or [SR], "chunk_s": args.chunk / SR,
         "pushes": args.pushes, "warmup": args.warmup, "ids_equal": bool(same), "tokens": tokens, "runs": 1}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v)}
        rows.append(f"{S:8d}  {k:14s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {len(v):4d}")
    r["torch_over_channels"] = round(r["torch_in_front"]["median_ms"] / r[wire]["median_ms"], 3)
    rows.append(f"{S:8d}  median step with {S} torch downmixes in front / with {ch}-channel sessions: {r['torch_over_channels']:.3f}; "
                f"ids equal: {same}; one run")
    what = ",".join(map(str, rates)) if rates else "the codec's rate"
    table = [f"encode sessions fed interleaved {ch}-channel {fmt} frames at {what}, 0.32 s pushes, starts staggered by a third of a push, 80 mel / "
             f"8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py --sessions {S} --channels {ch} --sample-format {fmt}" +
             (f" --sample-rate {what})" if rates else ")"),
             f"wall time of one step (one push for every stream) incl. host synchronisation, {args.pushes - args.warmup} steady-state steps, the two "
             "forms interleaved in one process;",
             f"{wire} = open(sample_format=\"{fmt}\", channels={ch}): one convert launch per step, the downmix inside it; torch_in_front = mono f32 "
             "sessions, the format's conversion and .sum(1) / C per slot",
             "sessions  form            median ms     p10 ms     p90 ms     n"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))
    assert same, "the ids of the channel-carrying sessions differ from those of the torch downmix in front"


def sessions_park_section():
    import bench_park
    S, n, pushes = args.sessions, args.chunk, 12
    audio = torch.randn(S, pushes * n, device=dev) * 0.1
    pool = codec.encode_sessions(slots=S, max_push_samples=n)
    slots = [pool.open() for _ in range(S)]
    for j in range(pushes):                                                  # steady state: every slot holds its live window
        pool.push({s: audio[i, j * n:(j + 1) * n] for i, s in enumerate(slots)})
    r, rows, slots = bench_park.measure(pool, slots)
    table = [f"snapshot + restore of {S} encode sessions in steady state ({n / SR:.2f} s pushes), 80 mel / 8 groups / 70 channels / 20 layers, "
             f"cap {pool.cap} (tools/bench_stream_encode.py --sessions {S} --park)",
             f"wall time of one snapshot of all sessions and one restore of all of them incl. host synchronisation, {r['cycles']} cycles, the two "
             "interleaved in one process, equal words checked;",
             "one_launch = pool.park + pool.restore (ONE dmel_stream_pack_items launch each); torch_slices = a slice .clone() per tensor per slot "
             "and a cat, and a slice copy per tensor back",
             "sessions  way            median us      p10 us      p90 us     n  bytes moved      GB/s"] + rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(table) + "\n\n")
    print("\n".join(table), file=sys.stderr)
    print(json.dumps(r))


if args.park and not args.sessions:
    ap.error("--park needs --sessions")
if args.voice and not args.sessions:
    ap.error("--voice needs --sessions")
if args.dtmf and not args.sessions:
    ap.error("--dtmf needs --sessions")
if args.level and not args.sessions:
    ap.error("--level needs --sessions")
if args.sessions and args.level:
    sessions_level_section()
    sys.exit(0)
if args.echo and not args.sessions:
    ap.error("--echo needs --sessions")
if args.sessions and args.echo:
    sessions_echo_section()
    sys.exit(0)
if args.conceal and not args.sessions:
    ap.error("--conceal needs --sessions")
if args.sessions and args.conceal:
    sessions_conceal_section()
    sys.exit(0)
if args.denoise and not args.sessions:
    ap.error("--denoise needs --sessions")
if args.sessions and args.denoise:
    sessions_denoise_section()
    sys.exit(0)
if args.sessions and (args.voice or args.dtmf):
    sessions_detector_section("voice" if args.voice else "dtmf")
    sys.exit(0)
if args.sessions and args.park:
    sessions_park_section()
    sys.exit(0)
if args.channels != 1 and not args.sessions:
    ap.error("--channels needs --sessions")
if args.sessions and args.channels > 1:
    sessions_channels_section()
    sys.exit(0)
if args.sessions and args.sample_format != "f32":
    sessions_pcm_section()
    sys.exit(0)
if args.sessions and rates:
    sessions_resample_section()
    sys.exit(0)
if args.sessions:
    sessions_section()
    sys.exit(0)
if args.sample_rate:
    resample_section()
    sys.exit(0)

rows, result = [], {"chunk_samples": args.chunk, "chunk_s": args.chunk / SR, "pushes": args.pushes, "warmup": args.warmup, "batch": {}}
for B in [int(b) for b in args.batches.split(",")]:
    audio = torch.randn(B, args.pushes * args.chunk, device=dev) * 0.1
    encs = {"one_launch": codec.streaming_encoder(B), "layered": codec.streaming_encoder(B)}
    ms = {k: [] for k in encs}
    same = True
    for i in range(args.pushes):
        chunk = audio[:, i * args.chunk:(i + 1) * args.chunk]
        order = ("one_launch", "layered") if i % 2 == 0 else ("layered", "one_launch")       # neither path always goes first
        got = {}
        for k in order:
            t, got[k] = timed_push(encs[k], chunk, k == "layered")
            if i >= args.warmup:
                ms[k].append(t)
        same = same and torch.equal(got["one_launch"], got["layered"])
    os.environ.pop("DMEL_WAVENET_STREAM_FUSED", None)
    for e in encs.values():
        e.finish()
    lens = torch.full((B,), audio.shape[1], device=dev)
    whole = []
    for i in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codec.encode(audio, lens)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    r = {"ids_equal": bool(same), "encode_whole_clip_ms": round(statistics.median(whole[2:]), 3), "clip_s": audio.shape[1] / SR}
    for k, v in ms.items():
        med = statistics.median(v)
        r[k] = {"median_ms": round(med, 3), "p10_ms": round(pct(v, 0.1), 3), "p90_ms": round(pct(v, 0.9), 3), "n": len(v),
                "audio_s_per_s": round(B * args.chunk / SR / (med / 1e3), 1)}
        rows.append(f"{B:5d}  {k:10s}  {med:9.3f}  {pct(v, 0.1):9.3f}  {pct(v, 0.9):9.3f}  {r[k]['audio_s_per_s']:11.1f}  {len(v):4d}")
    r["layered_over_one_launch"] = round(r["layered"]["median_ms"] / r["one_launch"]["median_ms"], 2)
    rows.append(f"{B:5d}  encode() of the whole {r['clip_s']:.2f} s clip: {r['encode_whole_clip_ms']:.3f} ms; ids equal: {same}")
    result["batch"][str(B)] = r

table = ["streaming encode, 0.32 s pushes of 24 kHz audio, 80 mel / 8 groups / 70 channels / 20 layers (tools/bench_stream_encode.py)",
         f"per-push wall time incl. host synchronisation, {args.pushes - args.warmup} steady-state pushes, the two paths interleaved in one process",
         "batch  path        median ms     p10 ms     p90 ms  audio-s / s     n"] + rows
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(table) + "\n")
print("\n".join(table), file=sys.stderr)
print(json.dumps(result))
