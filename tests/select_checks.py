"""What tests/test_gpu_select.py (device) and tests/test_emu_select.py (wavefront emulator) both assert about trial compression
(include/blosc_gpu_select.h): several parameter sets per chunk, the smallest result is written.  The yardstick is never the code under
test: a candidate's expected chunk is what the EXISTING blosc_gpu_compress_batch writes for that chunk alone with that setting and
destsize nbytes + 16 (params_checks.Calls.old_batch), the expected winner is the argmin of those sizes - the lowest index on a tie -
computed here, the expected container is packed_checks.expected_container over the winners' chunks."""
import ctypes as C

import numpy as np

import params_checks as pc
from batch_bounds_checks import check_written, guarded_slots
from getitem_ranges_checks import SENTINEL
from helpers import DATASETS, header
from packed_checks import FILL, GUARD, capacity_cases, check_chunks_decode, check_container, host_offsets, mixed_batch

Setting = pc.Setting


def candidates():
    """check 1's list: no filter, byte shuffle, bitshuffle, another codec twice - and the first setting again, which ties with index 0
    on every chunk and must never win"""
    return [Setting(b"lz4", 0, 1, 5), Setting(b"lz4", 1, 8, 5), Setting(b"lz4", 2, 8, 5), Setting(b"zstd", 1, 8, 3), Setting(b"blosclz", 1, 8, 5),
            Setting(b"lz4", 0, 1, 5)]


NONDETERMINISTIC = [Setting(b"lz4", 1, 8, 5), Setting(b"lz4hc", 1, 8, 5), Setting(b"zlib", 1, 8, 5), Setting(b"zstd", 1, 8, 7), Setting(b"lz4", 0, 1, 5)]


def text_like(n, seed=5):
    """words of a small vocabulary in random order: matches at byte distances that are no multiple of 8 - no filter beats both"""
    rng = np.random.default_rng(seed)
    words = [b"chunk ", b"filter ", b"candidate ", b"shuffle ", b"the ", b"of ", b"wave ", b"a ", b"smallest ", b"answer, ", b"is ", b"kept.\n"]
    out = b"".join(words[int(k)] for k in rng.integers(0, len(words), n // 2 + 8))
    return np.frombuffer(out[:n], np.uint8).copy()


def select_hosts(sizes):
    """packed_checks.mixed_batch(sizes) - bench19, a random walk, zeros, 0 and 100 random bytes, linspace, random bytes - plus small
    integers and text: what bitshuffle and no filter are for"""
    return mixed_batch(sizes) + [DATASETS["smallints"](sizes[6] * 2), text_like(sizes[6] * 2)]


INCOMPRESSIBLE, EMPTY, TINY = 6, 3, 4      # indices in select_hosts: random bytes; nbytes 0; 100 bytes (MEMCPYED on the host)


def tables(per_chunk):
    """[[row, ...] per chunk] -> (cand_first, rows)"""
    first, rows = [0], []
    for c in per_chunk:
        rows += list(c)
        first.append(len(rows))
    return first, rows


def argmin(sizes):
    """the winner of include/blosc_gpu_select.h over a list of answers: the smallest positive one, the lowest index on a tie; -1: none"""
    best = -1
    for k, s in enumerate(sizes):
        if s > 0 and (best < 0 or s < sizes[best]): best = k
    return best


class Calls(pc.Calls):
    def __init__(self, pkgmod, lib, mem, blocksize):
        super().__init__(pkgmod, lib, mem, blocksize)
        pkgmod.declare_select(lib)

    def select_batch(self, hosts, first, rows, caps=None, stream=None):
        """one blosc_gpu_compress_batch_select into guarded slots of one sentinel-filled buffer -> (results, choices, candidate answers,
        image, offsets of the destinations)"""
        n, sizes = len(hosts), [h.size for h in hosts]
        caps = [z + 16 for z in sizes] if caps is None else caps
        at, total = guarded_slots([max(c, z + 16) for c, z in zip(caps, sizes)])
        h, base = self.mem.filled(total, SENTINEL)
        b = self.pkg.DeviceBatch(self.src(hosts), sizes, [base + a for a in at], caps)
        for k in range(n): b.res[k] = -777
        assert b.compress_select(first, rows, stream=stream, lib=self.lib) == 0
        return b.results(), b.choices(), b.candidate_results(), self.mem.get(h)[:total], at

    def select_packed(self, hosts, first, rows, align, destsize, sizing=False, stream=None):
        """one blosc_gpu_compress_packed_select (sizing: dest NULL, destsize 0) -> (offsets, results, choices, candidate answers, buffer)"""
        b = self.pkg.PackedBatch(len(hosts), lib=self.lib)
        h, base = self.mem.filled(destsize + GUARD, FILL)
        assert b.compress_select(self.src(hosts), [x.size for x in hosts], first, rows, None if sizing else base, 0 if sizing else destsize, align, stream=stream) == 0
        return b.offsets(), b.results(), b.choices(), b.candidate_results(), self.mem.get(h)[:destsize + GUARD]


def yardstick(calls, hosts, settings):
    """ref[s][d]: data set d through the existing call with setting s, one call per setting"""
    return pc.reference_chunks(calls, hosts, settings)


def winners(ref, n):
    """(choice, chunk) per data set out of ref[s][d]"""
    choice = [argmin([ref[s][d].size for s in range(len(ref))]) for d in range(n)]
    return choice, [ref[choice[d]][d] for d in range(n)]


# ---- check 1 ----
def check_inputs_of_the_first_check(hosts, settings, ref):
    """what the data sets and the list are chosen for, shown by the existing calls alone"""
    n, S = len(hosts), len(settings)
    choice, _ = winners(ref, n)
    sizes = [[ref[s][d].size for s in range(S)] for d in range(n)]
    assert len(set(choice)) >= 3, ("the winners name fewer than three candidates", choice)
    assert all(sizes[d][S - 1] == sizes[d][0] for d in range(n)) and S - 1 not in choice, "the duplicate ties with index 0 and never wins"
    z = hosts[INCOMPRESSIBLE].size
    assert z >= 128 and sizes[INCOMPRESSIBLE] == [z + 16] * S and choice[INCOMPRESSIBLE] == 0, sizes[INCOMPRESSIBLE]
    assert hosts[EMPTY].size == 0 and sizes[EMPTY] == [16] * S and hosts[TINY].size == 100 and sizes[TINY] == [116] * S
    assert choice[EMPTY] == 0 and choice[TINY] == 0
    return choice


def check_deterministic(calls, hosts, settings, ref, oracle, reflib, aligns=(1, 16), stream=None, keep=None):
    """stream: the caller's stream of the select calls (default the NULL stream); keep: a dict that receives what they gave"""
    n, S = len(hosts), len(settings)
    want_choice, want = winners(ref, n)
    first, rows = tables([[calls.row(s) for s in settings]] * n)
    flat = [ref[s][d].size for d in range(n) for s in range(S)]
    res, choice, cand, image, at = calls.select_batch(hosts, first, rows, stream=stream)
    if keep is not None:
        keep.update(batch_cbytes=np.array(res, np.int64), batch_choice=np.array(choice, np.int64), batch_candidates=np.array(cand, np.int64), batch_image=image)
    assert cand == flat, ("candidate answers", [(e, a, b) for e, (a, b) in enumerate(zip(cand, flat)) if a != b][:6])
    assert choice == want_choice and res == [c.size for c in want], (choice, want_choice, res)
    check_written(image, at, want, "deterministic candidates, batch form", [h.size + 16 for h in hosts])
    # the rows of the 0-byte and the 100-byte chunk through the _params call: the same chunks
    for d in (EMPTY, TINY):
        r1, im1, at1 = calls.new_batch([hosts[d]], [rows[first[d]]], stream=stream)
        assert r1 == [res[d]] and np.array_equal(im1[at1[0]:at1[0] + r1[0]], image[at[d]:at[d] + res[d]])
    for align in aligns:
        need = host_offsets([c.size for c in want], align)[-1]
        off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, need, stream=stream)
        if keep is not None:
            keep.update({f"packed_offsets_align{align}": np.array(off, np.int64), f"packed_cbytes_align{align}": np.array(cb, np.int64), f"packed_container_align{align}": buf,
                         f"packed_choice_align{align}": np.array(choice, np.int64), f"packed_candidates_align{align}": np.array(cand, np.int64)})
        assert cand == flat and choice == want_choice, (align, choice, want_choice)
        check_container(buf, off, cb, want, align, need, ("deterministic candidates, packed form", align))
    check_chunks_decode([buf[off[d]:off[d] + cb[d]] for d in range(n)], hosts, oracle, reflib)


# ---- check 2 ----
def check_one_candidate_per_chunk(calls, hosts, settings, align=16):
    n = len(hosts)
    rows = [calls.row(settings[d % len(settings)]) for d in range(n)]
    first = list(range(n + 1))
    res0, image0, at0 = calls.new_batch(hosts, rows)
    res, choice, cand, image, at = calls.select_batch(hosts, first, rows)
    assert res == res0 and cand == res0 and choice == [0] * n and at == at0, (res, res0, choice)
    assert np.array_equal(image, image0), "batch form: the bytes differ from blosc_gpu_compress_batch_params'"
    need = host_offsets(res0, align)[-1]
    off0, cb0, buf0 = calls.new_packed(hosts, rows, align, need)
    off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, need)
    assert off == off0 and cb == cb0 and cand == cb0 and choice == [0] * n
    assert np.array_equal(buf, buf0), "packed form: the container differs from blosc_gpu_compress_packed_params'"


# ---- check 3 ----
def seventy(blocksizes=(128, 256, 384, 512, 1024, 2048, 4096)):
    """clevels 0 ... 9 times seven blocksizes, blocks never split (a forced blocksize stays what it is): fewer block starts as the
    list goes on, so the smallest chunks are at its end"""
    assert len(blocksizes) == 7
    return [Setting(b"lz4", 1, 4, clevel, splitmode=pc.NEVER_SPLIT, blocksize=bs) for bs in blocksizes for clevel in range(10)]


def check_ragged(calls, tiny, two, settings70, pair, align=16):
    """chunks with 0, 1, 70, 2 and 0 candidates in one call; the 70 belong to one tiny chunk, so a wave strides its range"""
    assert len(settings70) == 70
    hosts = [two, two, tiny, two, tiny]
    lists = [[], [pair[1]], settings70, pair, []]
    ref70 = [calls.old_batch([tiny], s)[0] for s in settings70]
    refp = [calls.old_batch([two], s)[0] for s in pair]
    assert len({c.size for c in ref70}) > 2, "the 70 candidates all have one size"
    w70, wp = argmin([c.size for c in ref70]), argmin([c.size for c in refp])
    assert w70 >= 64, ("the winner of the 70 lies in the first round of the wave's stride", w70)
    want_choice = [-1, 0, w70, wp, -1]
    spans = [None, refp[1], ref70[w70], refp[wp], None]
    want_res = [-10, refp[1].size, ref70[w70].size, refp[wp].size, -10]
    flat = [refp[1].size] + [c.size for c in ref70] + [c.size for c in refp]
    first, rows = tables([[calls.row(s) for s in l] for l in lists])
    assert first == [0, 0, 1, 71, 73, 73]
    res, choice, cand, image, at = calls.select_batch(hosts, first, rows)
    assert cand == flat, [(e, a, b) for e, (a, b) in enumerate(zip(cand, flat)) if a != b][:6]
    assert choice == want_choice and res == want_res, (choice, want_choice, res, want_res)
    check_written(image, at, spans, "ragged tables, batch form", [h.size + 16 for h in hosts])
    placed = [np.empty(0, np.uint8) if s is None else s for s in spans]
    need = host_offsets([c.size for c in placed], align)[-1]
    off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, need)
    assert cand == flat and choice == want_choice and cb == want_res, (choice, cb)
    want_off, _, want_buf = __import__("packed_checks").expected_container(placed, align, need)
    assert off == want_off and np.array_equal(buf, want_buf), (off, want_off)


THREE = [Setting(b"lz4", 0, 1, 5), Setting(b"lz4", 1, 8, 5), Setting(b"lz4", 2, 4, 5)]


def many_hosts(n, size):
    """n chunks of `size` bytes cut out of text, a linear ramp of float64 and small integers in turn - one for each of THREE"""
    pools = [text_like(size * (n // 3 + 1)), DATASETS["linspace"](size * (n // 3 + 1)), DATASETS["smallints"](size * (n // 3 + 1))]
    order = [0, 1, 2, 1, 0, 2, 2]      # (no period of three: the winners do not line up with the tiles)
    return [pools[order[k % 7]][(k // 3) * size:(k // 3 + 1) * size] for k in range(n)]


def check_many_chunks(calls, hosts, three, align):
    """300 chunks of 3 candidates: 900 entries cross the layout's tiles of 256, losers on both sides of every tile boundary"""
    n = len(hosts)
    assert n * 3 > 3 * 256 and len(three) == 3
    ref = yardstick(calls, hosts, three)
    want_choice, want = winners(ref, n)
    assert len(set(want_choice)) == 3, ("every candidate wins somewhere", sorted(set(want_choice)))
    for edge in (256, 512, 768):      # the entries left and right of a tile boundary: at least one loser on either side
        assert any(want_choice[e // 3] != e % 3 for e in (edge - 2, edge - 1)) and any(want_choice[e // 3] != e % 3 for e in (edge, edge + 1))
    first, rows = tables([[calls.row(s) for s in three]] * n)
    need = host_offsets([c.size for c in want], align)[-1]
    off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, need)
    assert choice == want_choice, [(d, a, b) for d, (a, b) in enumerate(zip(choice, want_choice)) if a != b][:6]
    assert cand == [ref[s][d].size for d in range(n) for s in range(3)]
    check_container(buf, off, cb, want, align, need, "300 chunks of three candidates")
    return ref, want_choice, want


# ---- check 4 ----
def check_errors(calls, hosts, good, align=16):
    """bad rows among good ones: their codes in the candidate table, a good candidate wins; a chunk whose candidates all fail answers the
    first code, choice -1, takes no room, and its neighbours are written as if it were not there"""
    bad_clevel, snappy = calls.pkg.cparams(8, 10, 1, b"lz4", calls.blocksize), calls.pkg.cparams(8, 5, 1, 3, calls.blocksize)
    a, b, c = hosts[0], hosts[1], hosts[2]
    refa, refc = [calls.old_batch([a], s)[0] for s in good], [calls.old_batch([c], s)[0] for s in good]
    wa, wc = argmin([x.size for x in refa]), argmin([x.size for x in refc])
    g = [calls.row(s) for s in good]
    assert len(g) == 2
    lists = [[bad_clevel, g[0], snappy, g[1]], [snappy, bad_clevel], [g[0], g[1], bad_clevel]]
    first, rows = tables(lists)
    flat = [-10, refa[0].size, -5, refa[1].size, -5, -10, refc[0].size, refc[1].size, -10]
    want_choice, want_res = [(1, 3)[wa], -1, wc], [refa[wa].size, -5, refc[wc].size]
    res, choice, cand, image, at = calls.select_batch([a, b, c], first, rows)
    assert cand == flat and choice == want_choice and res == want_res, (cand, flat, choice, res)
    check_written(image, at, [refa[wa], None, refc[wc]], "errors, batch form", [h.size + 16 for h in (a, b, c)])
    need = host_offsets([refa[wa].size, refc[wc].size], align)[-1]
    off, cb, choice, cand, buf = calls.select_packed([a, b, c], first, rows, align, need)
    assert cand == flat and choice == want_choice and cb == want_res
    assert off == host_offsets(cb, align) and off[1] == off[2] and off[-1] == need
    f2, r2 = tables([lists[0], lists[2]])
    off2, cb2, _, _, buf2 = calls.select_packed([a, c], f2, r2, align, need)
    assert cb2 == [want_res[0], want_res[2]] and np.array_equal(buf, buf2), "the container differs from the one without the failing chunk"
    check_container(buf2, off2, cb2, [refa[wa], refc[wc]], align, need, "errors, the good chunks alone")


# ---- check 5 ----
def check_capacity_batch(calls, hosts, settings, ref):
    """destsize[i] = the winner's size, then one byte less: the candidate that wins is the argmin of the answers the yardstick sizes give
    under that limit (a candidate above it answers 0: no chunk of its source is smaller than its smallest), or nobody - answer 0, the
    destination untouched"""
    n, S = len(hosts), len(settings)
    choice0, want0 = winners(ref, n)
    first, rows = tables([[calls.row(s) for s in settings]] * n)
    for less in (0, 1):
        caps = [c.size - less for c in want0]
        answers = [[ref[s][d].size if ref[s][d].size <= caps[d] else 0 for s in range(S)] for d in range(n)]
        want_choice = [argmin(a) for a in answers]
        res, choice, cand, image, at = calls.select_batch(hosts, first, rows, caps=caps)
        assert cand == [x for a in answers for x in a], (less, "candidate answers")
        assert choice == want_choice and res == [a[c] if c >= 0 else a[0] for a, c in zip(answers, want_choice)], (less, choice, want_choice, res)
        assert want_choice == (choice0 if less == 0 else [-1] * n)
        check_written(image, at, [ref[c][d] if c >= 0 else None for d, c in enumerate(want_choice)], ("capacity, batch form", less), caps)


def check_capacity_packed(calls, hosts, settings, ref, align):
    n, S = len(hosts), len(settings)
    want_choice, want = winners(ref, n)
    first, rows = tables([[calls.row(s) for s in settings]] * n)
    flat = [ref[s][d].size for d in range(n) for s in range(S)]
    need = host_offsets([c.size for c in want], align)[-1]
    seen = None
    for name, destsize in capacity_cases(want, align):
        off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, destsize)
        assert off[-1] == need and choice == want_choice and cand == flat, (name, off[-1], need, choice)
        check_container(buf, off, cb, want, align, destsize, (name, align))
        if name == "the need": assert all(c > 0 for c in cb)
        if name == "nothing": assert not any(cb)
        seen = (off, choice, cand)
    off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, 0, sizing=True)
    assert (off, choice, cand) == seen and not any(cb) and np.all(buf == FILL), "the sizing call differs from the real one"


# ---- check 6 ----
def check_nondeterministic(calls, hosts, settings, oracle, reflib, align=16):
    """candidates whose sizes may differ from call to call: the winner is the minimum of THIS call's table"""
    n, S = len(hosts), len(settings)
    heads = [calls.old_batch(hosts, s) for s in settings]
    first, rows = tables([[calls.row(s) for s in settings]] * n)

    def check(chunks, res, choice, cand, what):
        assert len(cand) == n * S
        for d in range(n):
            mine = cand[d * S:(d + 1) * S]
            assert choice[d] == argmin(mine) >= 0 and res[d] == mine[choice[d]], (what, d, choice[d], mine, res[d])
            c = chunks[d]
            assert res[d] == header(c)["cbytes"] == c.size, (what, d, header(c))
            assert np.array_equal(c[:12], heads[choice[d]][d][:12]), (what, d, settings[choice[d]], "header bytes 0 ... 11")
        check_chunks_decode(chunks, hosts, oracle, reflib)

    res, choice, cand, image, at = calls.select_batch(hosts, first, rows)
    check_written(image, at, [int(r) for r in res], "the other settings, batch form: bytes around the chunks", [h.size + 16 for h in hosts])
    check([image[a:a + r] for a, r in zip(at, res)], res, choice, cand, "batch form")
    need = sum((h.size + 16 + align - 1) // align * align for h in hosts)
    off, cb, choice, cand, buf = calls.select_packed(hosts, first, rows, align, need)
    assert off == host_offsets(cb, align) and np.all(buf[need:] == FILL)
    check([buf[off[d]:off[d] + cb[d]] for d in range(n)], cb, choice, cand, "packed form")
    for d in range(n): assert not buf[off[d] + cb[d]:off[d + 1]].any(), d
    assert np.all(buf[off[-1]:] == FILL)
    return choice
