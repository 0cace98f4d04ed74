"""Plain definitions of what the scans under every build and export compute (agx_launch_exclusive_scan, agx_launch_exclusive_scan1: csrc/agx_kernels.hip), and the
table of sizes at which tests/test_gpu_primitives.py runs them.  numpy and integers only: nothing here is shared with the kernels or with tests/scan_shim.cpp."""
import numpy as np

BLOCK = 4096                      # elements per workgroup (AGX_SCAN_BLOCK)
AGG, PFX = 1 << 62, 2 << 62       # a descriptor's two published states (AGX_SCAN_AGG, AGX_SCAN_PFX); 0: not published
GUARD = 64                        # AGX_TEST_GUARD
GUARD_WORD = 0xA5A5A5A5


def exclusive_scan(a):
    """a: the n + 1 words the scan reads.  out[i] = (a[0] + .. + a[i - 1]) mod 2^32 for i = 0 .. n; a[n] reaches nothing."""
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)
    return ((c - a.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def block_prefixes(a):
    """The inclusive prefix (mod 2^32) behind each block of 4096 of the n + 1 words: what block b publishes for the blocks behind it."""
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)
    ends = np.minimum(np.arange(1, levels(len(a) - 1)[0] + 1, dtype=np.int64) * BLOCK, len(a)) - 1
    return (c[ends] & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def block_totals(a):
    nb = levels(len(a) - 1)[0]
    p = np.zeros(nb * BLOCK, np.uint64)
    p[:len(a)] = a
    return (p.reshape(nb, BLOCK).sum(axis=1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def levels(n):
    """(nb, nb2, launches) of the multi-launch scan of n elements: it scans n + 1."""
    nb = (n + 1 + BLOCK - 1) // BLOCK
    nb2 = (nb + BLOCK - 1) // BLOCK
    return nb, nb2, 1 if nb == 1 else 3 if nb2 == 1 else 5


def tmp_words(n):
    nb, nb2, _ = levels(n)
    return 2 * (nb + 1) + 2 * (nb2 + 1)


def iterations(nb, grid):
    """Blocks that workgroup 0 .. min(nb, grid) - 1 of the one-launch scan take: g, g + grid, g + 2 grid, .."""
    return [len(range(g, nb, grid)) for g in range(min(nb, grid))]


def lookback(flags, values, b):
    """Block b walks back from b - 1, adds what it meets and stops behind the first prefix (in front of block 0 lies a prefix of 0).
    flags[j] in (AGG, PFX).  Returns (exclusive prefix mod 2^32, descriptors read)."""
    total, read = 0, 0
    for j in range(b - 1, -1, -1):
        total += int(values[j])
        read += 1
        if flags[j] == PFX:
            break
    return total & 0xFFFFFFFF, read


def windows_read(read):
    """The look-back reads 64 descriptors at a time."""
    return (read + 63) // 64


def window(flags, values):
    """One window, lane 0 the nearest predecessor: what every lane contributes, and whether the walk ends here."""
    parts, met = [], False
    for f, v in zip(flags, values):
        parts.append(0 if met else int(v) & 0xFFFFFFFF)
        met = met or f == PFX
    return parts, met


# ---- the sizes of tests/test_gpu_primitives.py, each with the arm it is there for: (nb, nb2, launches of the multi-launch form) -------------------------------
SCAN_SIZES = {
    0: (1, 1, 1), 1: (1, 1, 1), 255: (1, 1, 1), 256: (1, 1, 1),
    4094: (1, 1, 1), 4095: (1, 1, 1),                         # n + 1 = 4096: the last one-block cases
    4096: (2, 1, 3),                                          # two blocks
    8191: (2, 1, 3), 8192: (3, 1, 3),
    65535: (16, 1, 3), 65536: (17, 1, 3),
    16777214: (4096, 1, 3), 16777215: (4096, 1, 3),           # the last two-level cases
    16777216: (4097, 2, 5),                                   # the smallest three-level scan: the second block of level two holds one sum
    16781312: (4098, 2, 5),
    20000001: (4883, 2, 5),
}
ALL_PATTERNS_UP_TO = 1 << 20                                  # above: ones, the steps, 32-bit random
STEP_AT = (4095, 4096, 4096 * 4096 - 1, 4096 * 4096)          # a single 1 here: the index behind it at which the output steps says which level dropped an offset
GRID_CAPS = (1, 2, 16, 63, 64, 65, 0)                         # 0: the launcher's own grid
OWN_GRID_BLOCKS = (65, 66, 129, 300)                         # at the launcher's own grid: the last block looks back over one full window, into a second, over two, into a fifth


def capped_blocks(grid):
    """Block counts for a one-launch scan on `grid` workgroups: the last workgroup idle, every one busy once, workgroup 0 twice, workgroup 0 three times."""
    return [nb for nb in (grid - 1, grid, grid + 1, 2 * grid + 1) if nb >= 1]


def n_for_blocks(nb, last=1234):
    """An n whose n + 1 words fill nb - 1 blocks and `last` words of the nb-th: the last block is partial."""
    return (nb - 1) * BLOCK + last - 1


def patterns_for(n):
    return ("ones", "step", "random") if n > ALL_PATTERNS_UP_TO else ("ones", "step", "product", "wrap", "random")


def make(pattern, n, tail, seed=1, step_at=None):
    """The n + 1 input words of a pattern; a[n] = tail."""
    rnd = np.random.RandomState(seed)
    if pattern == "ones":
        a = np.ones(n + 1, np.uint32)
    elif pattern == "step":
        a = np.zeros(n + 1, np.uint32)
        a[step_at] = 1
    elif pattern == "product":                                # mostly zero, values below 97: the side-id counts
        a = np.where(rnd.randint(0, 5, n + 1) == 0, rnd.randint(0, 97, n + 1), 0).astype(np.uint32)
    elif pattern == "wrap":
        a = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    elif pattern == "random":
        a = rnd.randint(0, 1 << 32, n + 1, dtype=np.uint64).astype(np.uint32)
    else:
        raise ValueError(pattern)
    a[n] = tail
    return a
