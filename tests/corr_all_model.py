"""The definition of srcdsp_corr_step_all: the application's loop of
FixedPatternCorrelator::step on the remainders (correlators.h:209-303), over
any correlator object with ``step(x) -> (found, corrIndex)`` and
``bit_samples()`` -- the oracle's, or the Python face's on clones -- and the
signals and cases the CPU and GPU tests of the call share."""
import numpy as np

TILE = 4096  # outputs per workgroup of the candidate pass


def step_all(cor, x, max_hits):
    """(indices, bits [k, N, 2], consumed) of one call on the samples `x`."""
    n, off, idx, bits = len(x), 0, [], []
    while off < n and len(idx) < max_hits:
        found, ci = cor.step(x[off:n])
        if not found:
            off = n
            break
        idx.append(off + ci)  # may be off - 1: the peak was the sample before this remainder
        bits.append(np.array(cor.bit_samples(), np.int16).reshape(-1, 2).copy())
        off += ci + 2
    b = np.stack(bits) if bits else np.zeros((0, cor.N, 2), np.int16)
    return np.array(idx, np.int64), b, off


def step_all_status(O, N, p, x):
    """getStatus of a fresh oracle correlator after one unlimited call on x."""
    r = O["fma"].corr(N, 1)
    r.set_pattern(p)
    step_all(r, x, len(x))
    return r.status()


def firing_points(cor, x):
    """Where the peak test fires on the undisturbed stream (no sample removed):
    the sample being processed, i.e. corrIndex + 1.  `cor` is a fresh oracle
    correlator with its pattern set; the literal test of correlators.h:262-268."""
    c, e = cor.registers(x)
    out = []
    for i in range(2, len(x)):
        if c[i - 1] > c[i - 2] and c[i - 1] > c[i]:
            corr, energy = np.sqrt(np.float64(c[i - 1])), np.sqrt(np.float64(e[i - 1]))
            if corr > energy * 2.7 and energy > 300:
                out.append(i)
    return out


def pattern(N, seed, amplitude=500):
    from srcdsp_amd.design import qpsk_pattern
    return qpsk_pattern(N, amplitude, seed=seed)


def signal(n, seed, bursts, gain=2, noise=125):
    """Noise uniform in +-noise with x[off + m] += gain p[m] for every (off, p)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-noise, noise + 1, size=(n, 2)).astype(np.int32)
    for off, p in bursts:
        lo, hi = max(off, 0), min(off + len(p), n)
        if lo < hi:
            x[lo:hi] += gain * p[lo - off:hi - off]
    return np.clip(x, -32768, 32767).astype(np.int16)


def run_calls(call, x, chunks, max_hits):
    """`x` taken in calls of `chunks` samples; a call that stops at max_hits is
    followed by calls on its remainder.  call(samples, max_hits) -> (indices,
    bits, consumed).  Returns [(start of the call, indices, bits, consumed)]."""
    out, pos = [], 0
    for m in chunks:
        end = pos + m
        while pos < end:
            idx, bits, used = call(x[pos:end], max_hits)
            out.append((pos, np.asarray(idx).tolist(), np.asarray(bits), int(used)))
            assert 1 <= used <= end - pos, (pos, end, used)
            pos += used
    return out


def same_calls(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[3] == w[3], (g[0], g[1], g[3], w[0], w[1], w[3])
        assert np.array_equal(g[2], w[2]), (g[0], "bitSamples")


GAPS = (0, 0, 0, 1, 1, 2, 5, 40)


def back_to_back(N, seed, start=500, gaps=GAPS, tail=300):
    """Nine preambles with `gaps` samples between them, at 8 x amplitude in
    +-200 noise: (pattern, x, the offsets)."""
    p = pattern(N, seed)
    offs, o = [], start
    for g in (0,) + tuple(gaps):
        o += g
        offs.append(o)
        o += N
    return p, signal(o + tail, seed + 1, [(f, p) for f in offs], gain=8, noise=200), offs


TILE_Q = (TILE, TILE + 1, TILE + 15, TILE + 16, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)
N_TILES = 3 * TILE + 500


def tile_row(N, q, seed):
    """A row whose first detection fires while sample q is processed (bursts
    are found at their last sample, so the test fires one later: off + N), with
    two more bursts behind it: (pattern, x)."""
    p = pattern(N, seed)
    return p, signal(N_TILES, seed + 50, [(q - N, p), (q + 700, p), (q + 2500, p)])


def cases():
    """The single-row cases: name -> (N, pattern, x, chunks, max_hits).  The
    oracle loop's detections of the b2b rows differ from their firing points
    (test_corr_all_model.py), which is what a kernel reporting every firing
    point fails."""
    out = {}
    for q in TILE_Q:  # sparse bursts; a detection in outputs 0, 1, 15, 16, 4095 of a tile and 0, 1 of the next
        p, x = tile_row(64, q, 600 + q % 97)
        out[f"tile_{q}"] = (64, p, x, [len(x)], 64)
    for N, seed in ((32, 1), (32, 4), (33, 1), (64, 3), (64, 1)):  # gaps 0, 1, 2
        p, x, _ = back_to_back(N, seed)
        out[f"b2b_{N}_{seed}"] = (N, p, x, [len(x)], 64)
    # the patch of the detection at TILE - 6 runs over the tile boundary, with a detection inside it
    p, x, _ = back_to_back(64, 1, start=TILE - 6 - 64)
    out["straddle"] = (64, p, x, [len(x)], 64)
    # b2b_32 in calls: the first ends 3 samples into a patch, the second on a
    # peak (the next call's first sample detects: index -1), then n < N twice
    p, x, _ = back_to_back(32, 1)
    out["split"] = (32, p, x, [535, 61, 5, 20, len(x) - 621], 64)
    p, x = tile_row(64, TILE, 611)
    out["short_calls"] = (64, p, x, [5, 20, 63, TILE, len(x) - TILE - 88], 64)
    p, x, _ = back_to_back(32, 1)
    out["max_hits_3"] = (32, p, x, [len(x)], 3)
    out["max_hits_exact"] = (32, p, x, [len(x)], 7)  # the row holds 7 detections: a remainder call finds none
    out["max_hits_1"] = (32, p, x, [700, len(x) - 700], 1)
    p, x = tile_row(33, TILE + 1, 633)
    out["n33_tiles"] = (33, p, x, [5000, len(x) - 5000], 64)
    return out
