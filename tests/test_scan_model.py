"""CPU model of the segment scan's decoupled look-back (mchecksum_gpu_ext.hip:
scan_block, seg_lookback), run under seeded interleavings of every scan
block's shared-memory steps, over SEVERAL launches on one workspace.

Each scan block is a generator that yields at every access to the
workspace's shared words -- the descriptors (flag, aggregate, inclusive
prefix), the call count `gen` and the fault claim -- and mirrors the device
code step by step: read gen; store the aggregate, then release-store the flag;
read a window of predecessors' flags (64 lanes on the device, `win` here) back
to the nearest inclusive prefix, waiting while a nearer block has not
published; sum; publish the inclusive prefix; the last block bumps gen.  A
bounded wait is a poll count.  Descriptors and gen persist from launch to
launch, as they do in the caller's workspace, and start as garbage.

What this checks is what a captured call needs: a graph replays the epoch it
captured, so every replay of one graph carries the same epoch while the
segment lengths -- device memory -- may have changed.  With flags tagged by
the epoch alone (rule="epoch", the code before this model existed) block b
takes block b - 1's inclusive prefix of the LAST replay for this one's
whenever it looks back before b - 1 has published; tagged by (epoch, gen)
(rule="gen") it cannot.  Lengths are chosen so that every block's inclusive
byte and chunk prefixes differ between consecutive launches (asserted), so a
stale prefix is never accidentally right.

The scheduler starts blocks in index order (a kernel's workgroups are
dispatched in order) and otherwise picks a started block at random, which is
fair: a waiting block's predecessor gets to run.  The directed order runs
every block, highest first, through its first window of flag reads before any
lower block has stored anything -- the order that needs no luck on the device,
since all blocks do the same work before publishing.
"""
import random

import pytest

CHUNK = 256 << 10
M64 = (1 << 64) - 1


def scan_key(epoch, gen):
    return (epoch ^ (gen * 0x9E3779B97F4A7C15) ^ 0xD1B54A32D192ED03) & M64


def tag_of(rule, epoch, gen):
    """The flag's upper 62 bits (the state sits in the low two)."""
    if rule == "epoch":
        return (epoch * 4) & M64
    return (scan_key(epoch, gen) << 2) & M64


def seg_chunks(n):
    return (n + CHUNK - 1) // CHUNK


def ragged(n):  # (the device also looks at the start's alignment: not modelled, it never changes)
    return int(n != 0 and n % 1024 != 0)


class Workspace:
    """The words that outlive a launch: 7 per scan block (flag, aggregate p c
    r, inclusive p c r), gen and the fault claim -- never cleared."""

    def __init__(self, nb, rnd):
        self.desc = [[rnd.getrandbits(64) for _ in range(7)] for _ in range(nb)]
        self.gen = rnd.getrandbits(64)
        self.claim = rnd.getrandbits(64)


def block_totals(lens, blk):
    nb = max(1, (len(lens) + blk - 1) // blk)
    tot = []
    for b in range(nb):
        ls = lens[b * blk:(b + 1) * blk]
        tot.append((sum(ls), sum(seg_chunks(n) for n in ls), int(any(ragged(n) for n in ls))))
    return tot


def true_exclusive(lens, blk):
    ex, p, c, r = [], 0, 0, 0
    for tp, tc, tr in block_totals(lens, blk):
        ex.append((p, c, r))
        p, c, r = p + tp, c + tc, r | tr
    return ex


def _block(ws, b, nb, tot, epoch, rule, win, deadline, res):
    """scan_block's wave 0 for block b: yields a label after each shared access."""
    tp, tc, tr = tot
    gen = ws.gen
    yield "gen"
    tag = tag_of(rule, epoch, gen)
    me = ws.desc[b]
    for w, v in ((1, tp), (2, tc), (3, tr)):
        me[w] = v
        yield "agg"
    if b == 0:
        for w, v in ((4, tp), (5, tc), (6, tr)):
            me[w] = v
            yield "incl"
    me[0] = tag | (2 if b == 0 else 1)  # release: after the words above
    yield "flag"
    sp = sc = sr = 0
    ok = True
    if b > 0:
        k, polls = b - 1, 0
        while True:
            lanes = [k - lane for lane in range(win)]
            state = []
            for n, idx in enumerate(lanes):
                f = ws.desc[idx][0] if idx >= 0 else tag | 2  # past block 0: the call's own tag
                state.append(f & 3 if (f & ~3 & M64) == tag else 0)
                if idx >= 0 and n + 1 < win and lanes[n + 1] >= 0:
                    yield "read"
            yield "window"
            S = next((n for n, s in enumerate(state) if s == 2), win)
            if any(s == 0 for s in state[:S]):  # a nearer block has not published yet
                polls += 1
                if polls >= deadline:
                    res["gave_up"] += 1
                    ok = False
                    break
                continue
            for n, idx in enumerate(lanes[:S + 1]):
                if idx < 0:
                    continue
                d = ws.desc[idx]
                o = 4 if n == S else 1
                vp = d[o]
                yield "read"
                vc = d[o + 1]
                yield "read"
                vr = d[o + 2]
                yield "read"
                sp, sc, sr = sp + vp, sc + vc, sr | vr
            if S < win:
                break
            k -= win
        for w, v in ((4, sp + tp), (5, sc + tc), (6, sr | tr)):
            me[w] = v
            yield "incl"
        me[0] = tag | 2
        yield "flag"
    res["ex"][b] = (sp, sc, 1 if sr else 0)
    res["gens"][b] = gen
    if not ok:  # report_scan_fault
        ws.claim = scan_key(epoch, gen)
        yield "claim"
    if b + 1 == nb:
        ws.gen = (gen + 1) & M64
        yield "bump"


def run_launch(ws, lens, epoch, rnd, rule="gen", blk=4, win=4, directed=False, deadline=20_000, max_steps=2_000_000):
    """One scan launch on the workspace; returns each block's exclusive
    (bytes, chunks, ragged), the gen each block read and the give-up count."""
    tot = block_totals(lens, blk)
    nb = len(tot)
    assert nb == len(ws.desc)
    res = dict(ex=[None] * nb, gens=[None] * nb, gave_up=0)
    gens = [_block(ws, b, nb, tot[b], epoch, rule, win, deadline, res) for b in range(nb)]
    live, started, steps = [], 0, 0

    def step(b):
        try:
            return next(gens[b])
        except StopIteration:
            live.remove(b)
            return None

    if directed:
        for b in range(nb):  # dispatched in order: each reads gen (no store yet)
            live.append(b)
            step(b)
        started = nb
        for b in range(nb - 1, 0, -1):  # highest first, through its first window of flags
            while b in live and step(b) != "window":
                pass
    while live or started < nb:
        n = len(live) + (started < nb)
        pick = rnd.randrange(n)
        if pick == len(live):  # the next block in index order starts
            live.append(started)
            started += 1
            step(live[-1])
        else:
            step(live[pick])
        steps += 1
        assert steps < max_steps, "no progress: a wait never ends"
    return res


# ---- lengths -----------------------------------------------------------------
# Launches alternate between two classes: "low" (each segment 0 -- about 30%
# -- or 1 chunk) and "high" (each segment 2 or 3 chunks).  Every block's
# totals in a high launch exceed the same block's in a low one, in bytes and
# in chunks, so every inclusive prefix differs between consecutive launches.

def draw_lens(rnd, nseg, high):
    if high:
        return [rnd.randrange(CHUNK + 1, 3 * CHUNK + 1) for _ in range(nseg)]
    ls = [0 if rnd.random() < 0.3 else rnd.choice([1, 7, 1024, 4096, CHUNK - 1, CHUNK, rnd.randrange(1, CHUNK + 1)])
          for _ in range(nseg)]
    if not any(ls):
        ls[rnd.randrange(nseg)] = 1024
    return ls


def inclusive(lens, blk):
    out, p, c = [], 0, 0
    for tp, tc, _ in block_totals(lens, blk):
        p, c = p + tp, c + tc
        out.append((p, c))
    return out


def assert_prefixes_differ(a, b, blk):
    for x, y in zip(inclusive(a, blk), inclusive(b, blk)):
        assert x[0] != y[0] and x[1] != y[1], "a stale prefix could be right by accident"


def replay_sequence(nb, seed, rule, directed, blk=4, win=4, replays=4):
    """An eager launch (epoch e0), then `replays` launches with one captured
    epoch e1, lengths changing every time; returns the number of blocks whose
    exclusive prefix was wrong, per launch."""
    rnd = random.Random(seed)
    nseg = (nb - 1) * blk + rnd.randrange(1, blk + 1)  # a partial last block too
    ws = Workspace(nb, rnd)
    e0 = rnd.getrandbits(61) | 1
    e1 = (e0 + 1 + rnd.randrange(1000)) & ((1 << 61) - 1)
    wrong, prev = [], None
    gen0 = ws.gen
    for n in range(1 + replays):
        lens = draw_lens(rnd, nseg, high=bool((n + seed) & 1))
        if prev is not None:
            assert_prefixes_differ(prev, lens, blk)
        prev = lens
        r = run_launch(ws, lens, e0 if n == 0 else e1, rnd, rule, blk, win, directed)
        assert r["gave_up"] == 0, "a look-back wait gave up"
        want = true_exclusive(lens, blk)
        wrong.append(sum(g != w for g, w in zip(r["ex"], want)))
        if rule == "gen":
            assert r["gens"] == [(gen0 + n) & M64] * nb, "blocks of one launch read different call counts"
        assert ws.gen == (gen0 + n + 1) & M64, "gen must rise by exactly one per launch"
    return wrong


NB = [1, 2, 5, 70]  # 70 blocks at a window of 4: 18 windows deep; 70 > 64 too


@pytest.mark.parametrize("nb", NB)
def test_replays_with_new_lengths_random_orders(nb):
    for seed in range(40):
        assert replay_sequence(nb, seed * 7919 + nb, "gen", directed=False) == [0] * 5, seed


@pytest.mark.parametrize("nb", NB)
def test_replays_with_new_lengths_directed_order(nb):
    for seed in range(40):
        assert replay_sequence(nb, seed * 104729 + nb, "gen", directed=True) == [0] * 5, seed


@pytest.mark.parametrize("win,blk", [(1, 1), (2, 3), (64, 4)])
def test_other_window_and_block_sizes(win, blk):
    for nb in (2, 5, 70):
        for seed in range(6):
            for directed in (False, True):
                assert replay_sequence(nb, seed + 31 * nb, "gen", directed, blk, win) == [0] * 5


@pytest.mark.parametrize("nb", [2, 5, 70])
def test_epoch_only_flags_take_a_stale_prefix(nb):
    """Teeth: the same model with the flags tagged by the epoch alone.  The
    eager launch and the first replay (a fresh epoch each) are right; from the
    second replay on, under the directed order, every block past 0 takes its
    predecessor's flag of the replay before for a current one.  (Its prefix
    words are read a few steps later: a block whose predecessor has stored the
    new ones by then -- block 0 stores them first thing -- is right by luck,
    which is all the epoch-only rule ever had.)"""
    for seed in range(10):
        wrong = replay_sequence(nb, seed * 13 + nb, "epoch", directed=True)
        assert wrong[:2] == [0, 0], wrong
        assert sum(wrong[2:]) > 0, wrong
        if nb > 2:
            assert all(w > 0 for w in wrong[2:]), wrong


def test_epoch_only_flags_fail_under_random_orders_too():
    """No directed order is needed: at 70 blocks some block looks back early in
    nearly every random order."""
    bad = sum(any(replay_sequence(70, seed, "epoch", directed=False)[2:]) for seed in range(10))
    assert bad >= 8, bad


def test_bounded_wait_gives_up_and_claims():
    """A block that never publishes (the test build's scanstall): its successor
    polls out its deadline, gives up and claims the call's key; gen still
    moves."""
    rnd = random.Random(5)
    ws = Workspace(3, rnd)
    lens = draw_lens(rnd, 12, high=True)
    tot = block_totals(lens, 4)
    res = dict(ex=[None] * 3, gens=[None] * 3, gave_up=0)
    gen0, epoch = ws.gen, 12345
    for b in (0, 2):  # block 1 never runs
        for _ in _block(ws, b, 3, tot[b], epoch, "gen", 4, 50, res):
            pass
    assert res["gave_up"] == 1 and ws.claim == scan_key(epoch, gen0) and ws.gen == (gen0 + 1) & M64
