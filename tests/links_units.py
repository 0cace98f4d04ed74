"""Hand-made stretch tables for the mate-links tests (tests/test_links_cases.py, tests/test_gpu_links.py): the shapes of a record layout that the owners, the classes and
the hash table can go wrong on.  Every table is valid for any unit of n_pos positions (main ids only: a main id is its position)."""
import path_model as PM

EVERY_BASE_MAX = 1024      # records of the every-base table at most (the model loops over them)


def links_tables(n_pos):
    """name -> stretch table.
      interleaved   three records whose stretches take turns along the unit, eight positions each and eight positions nobody's after every third: neighbouring stretches
                    belong to different records, so short fragments already link, in both directions
      every_base    every position (of the first EVERY_BASE_MAX) a record of its own: every fragment longer than one base is a link, the links are many and each has few pairs
      stacked       record 1 over the whole unit, records 0 and 2 both over its second quarter: 0 owns the quarter, 2 owns nothing and all its bases are shadowed, 1's
                    bases in the quarter are shadowed too; links (1, 0) and (0, 1)
      empty         no record
      one_record    one record over the whole unit: no link"""
    blocks = [(x, min(x + 7, n_pos - 1)) for x in range(0, n_pos, 8)]
    inter = [[], [], []]
    for i, (a, b) in enumerate(blocks):
        if i % 4 < 3:
            inter[i % 4].append((a, b))

    def rec(pieces):
        st, at = [], 0
        for a, b in pieces:
            st.append((a, b, at, 0))
            at += b - a + 1
        return (at, st)
    q = n_pos // 4
    n_every = min(n_pos, EVERY_BASE_MAX)
    return {
        "interleaved": PM.stretches([rec(p) for p in inter]),
        "every_base": PM.stretches([(1, [(x, x, 0, 0)]) for x in range(n_every)]),
        "stacked": PM.stretches([rec([(q, 2 * q - 1)]), rec([(0, n_pos - 1)]), rec([(q, 2 * q - 1)])]),
        "empty": PM.stretches([]),
        "one_record": PM.stretches([rec([(0, n_pos - 1)])]),
    }
