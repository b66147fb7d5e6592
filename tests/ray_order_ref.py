"""Plain restatement, in Python integers and numpy, of the pixel-major ray order of a launch set (vr_internal.h
"pixel-major ray order"; vr_regroup_kernel in vr_raycast.hip): what the index must hold, given what the pre-pass noted.

A launch set of set_frames frames of one camera has n = patches * set_frames work items, item q = patch * set_frames +
frame.  The pre-pass notes, per item, the 64-bit ballot of the patch's live rays in that frame (bit px = 8 * row +
column of the patch) and the position `first` of the item's first record in the ray lists; the records of an item lie
at first, first + 1, ... in ascending px.  The index holds, per patch with a live ray, one RUN: the positions of the
patch's live rays ordered by pixel first, frame second, padded with PM_NONE to a multiple of the group.  Runs of patch
p go to index list p % LISTS, in any order (they are appended through an atomic counter).

tests/test_ray_order_ref.py proves this module without a GPU; tests/test_gpu_ray_order.py holds the device to it."""
import numpy as np

LISTS = 8                    # kLiveLists
PM_NONE = 0xFFFFFFFF         # kPmNone
MAX_FRAMES = 256             # kMaxBatchFrames
GROUPS = (1, 32, 64)         # VRHIP_PM_GROUP


def popcount(x):
    return bin(int(x)).count("1")


def live_list_cap(n_items):
    """Records per ray list: ceil(n / 8) items of at most 64 records."""
    return ((n_items + LISTS - 1) // LISTS) * 64


def pm_list_cap(n_items, set_frames, bits=32):
    """Entries per index list, as the device computes it: in `bits`-bit unsigned arithmetic (None: unbounded)."""
    v = 8 * n_items + 64 * set_frames
    return v if bits is None else v & ((1 << bits) - 1)


def pm_block_words(n_items, set_frames):
    """Words of the whole block, in 64 bits on the host."""
    return 3 * n_items + LISTS * (8 * n_items + 64 * set_frames)


def block_layout(n_items, set_frames):
    """The block's parts as (name, first word, end word), in the order they lie in memory."""
    parts, at = [], 0
    for name, words in [("ballots", 2 * n_items), ("first", n_items)] + \
                       [("index%d" % k, pm_list_cap(n_items, set_frames, None)) for k in range(LISTS)]:
        parts.append((name, at, at + words))
        at += words
    return parts


def padded_length(total, group):
    """A run of `total` entries padded to a multiple of the group (a power of two); an empty run stays empty."""
    assert group in GROUPS
    return (total + group - 1) // group * group


def pixel_of_bit(col, row, px):
    """Frame pixel (gx, gy) of ballot bit px of the patch in column col, row `row`: the pre-pass's lane px handles
    pixel (8 col + (px & 7), 8 row + (px >> 3)) (vr_dda_prepass_kernel: lx = lane & 7, ly = lane >> 3)."""
    return 8 * col + (px & 7), 8 * row + (px >> 3)


def expected_run(ballots, firsts):
    """The run of one patch: ballots[f], firsts[f] for f in 0 .. set_frames - 1 -> list of (position, px, f), pixel
    outer, frame inner, where the bit is set."""
    run = []
    for px in range(64):
        below = (1 << px) - 1
        for f, (b, first) in enumerate(zip(ballots, firsts)):
            b = int(b)
            if (b >> px) & 1:
                run.append((int(first) + popcount(b & below), px, f))
    return run


def brute_force_run(ballots, firsts):
    """The same, by enumeration: the records of frame f are numbered first[f], first[f] + 1, ... over its set bits in
    ascending px; all of them sorted by (px, f)."""
    recs = []
    for f, (b, first) in enumerate(zip(ballots, firsts)):
        at = int(first)
        for px in range(64):
            if (int(b) >> px) & 1:
                recs.append((px, f, at))
                at += 1
    return [(at, px, f) for px, f, at in sorted(recs)]


def expected_runs(set_frames, ballot, first, group):
    """Every patch's padded run: {patch: uint32 array}, patches without a live ray left out.  ballot, first: per work
    item, item q = patch * set_frames + frame."""
    n = len(ballot)
    assert n % set_frames == 0 and len(first) == n
    runs = {}
    for p in range(n // set_frames):
        q0 = p * set_frames
        run = [at for at, _, _ in expected_run(ballot[q0:q0 + set_frames], first[q0:q0 + set_frames])]
        if run:
            runs[p] = np.array(run + [PM_NONE] * (padded_length(len(run), group) - len(run)), dtype=np.uint32)
    return runs


def regroup_walk(set_frames):
    """vr_regroup_kernel's walk over the 64 * set_frames (pixel, frame) pairs, restated in integers: lane l starts at
    (l / sf, l % sf) and advances by 64 pairs per step with a carry, no division in the loop.  Yields, per step, the
    list of the 64 lanes' (px, f)."""
    sf = set_frames
    dq, dr = 64 // sf, 64 % sf
    px = [lane // sf for lane in range(64)]
    f = [lane % sf for lane in range(64)]
    for _ in range(sf):
        yield list(zip(px, f))
        for lane in range(64):
            px[lane] += dq
            f[lane] += dr
            if f[lane] >= sf:
                f[lane] -= sf
                px[lane] += 1


def split_runs(entries, runs_of_list):
    """Split one index list into the runs it is made of: entries (uint32 array) against {patch: padded run} of the
    patches that belong to this list.  A run starts with a position (never PM_NONE) and no two patches share a
    position, so the first entry names the patch.  Returns the patches in the order their runs lie in the list; raises
    AssertionError where the list is not a concatenation of whole expected runs."""
    by_head = {int(r[0]): p for p, r in runs_of_list.items()}
    assert len(by_head) == len(runs_of_list), "two patches of one list start at the same record"
    order, at = [], 0
    while at < len(entries):
        head = int(entries[at])
        assert head != PM_NONE, "padding at entry %d where a run must start" % at
        assert head in by_head, "entry %d (position %d) starts no patch's run" % (at, head)
        p = by_head[head]
        want = runs_of_list[p]
        got = entries[at:at + len(want)]
        assert len(got) == len(want) and np.array_equal(got, want), \
            "patch %d: run at entry %d differs from the restatement:\n got  %s\n want %s" % (p, at, got[:96], want[:96])
        order.append(p)
        at += len(want)
    return order
