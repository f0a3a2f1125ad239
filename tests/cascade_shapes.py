"""The cascade launch groups that tests/test_gpu_cascade_forms.py builds, as (section count, chains, lanes per chain).

The device does not say which cascade kernel a launch took, so the GPU tests are tied to the rule instead: cascade_groups
(avdsp_amd/csrc/avdsp_plan_layout.h) gives a group P = pow2ceil(sections) lanes per chain, raised to a 16-lane row -- biquad_row,
biquad_row_i64 -- while chains * 16 <= 65536.  tests/test_plan_layout.py asserts on the CPU that the rule gives exactly the P listed
here, and that the narrow groups hold no biquad_row records; the GPU tests import the same lists.  If the threshold moves, the CPU
test fails and says that the GPU tests no longer reach biquad_pipe<FMT, 1 | 2 | 4 | 8>."""

NARROW_CHAINS = 4097            # the smallest group that leaves the 16-lane rows: 4097 * 16 > 65536

# one group per case of test_narrow_forms: P = 1, 2, 4, 4, 8, 8, 8 (three cases of sections < P)
NARROW = [(1, NARROW_CHAINS, 1), (2, NARROW_CHAINS, 2), (3, NARROW_CHAINS, 4), (4, NARROW_CHAINS, 4),
          (5, NARROW_CHAINS, 8), (7, NARROW_CHAINS, 8), (8, NARROW_CHAINS, 8)]

# the Inf / NaN cases (format 6): sub-row chains of four and of eight lanes, a full lane group and sections < P of each
NARROW_REPLAY = [(3, NARROW_CHAINS, 4), (4, NARROW_CHAINS, 4), (7, NARROW_CHAINS, 8), (8, NARROW_CHAINS, 8)]

# several groups in one core: two narrow groups of different P beside a handful of chains of three other section counts, which
# the merged row table takes
MIXED = [(2, NARROW_CHAINS, 2), (5, NARROW_CHAINS, 8), (6, 3, 16), (9, 2, 16), (16, 2, 16)]

# the row kernels at every block length: chains of 1 .. 16 sections (n: the plain chains; the FIR-feeding and the two-STORE chains
# of the GPU test join the groups of their section counts, which only makes them larger -- and 4096 is far)
ROWS = [(nsec, 1, 16) for nsec in range(1, 17)]


def narrow_block_lengths(nsec, P, trimmed=False):
    """Every block length a narrow case runs, in order: 1 .. NB (bs + 11) ascending with NB = P and bs = biquad_pipe's first steady
    batch (fill-only blocks, the first steady triple, a second one, every exit from the loop), then one-frame hand-overs of x1 / y1,
    then a block longer than one launch.  `trimmed`: the ascending list ends at NB (bs + 10), the first length whose steady loop
    (batches bs .. be = (B / NB - 4) / 3 * 3) makes two turns.  Returns (lengths, the number of ascending ones)."""
    nb = P
    bs = -(-(-(-(2 * nsec - 1) // nb)) // 3) * 3
    top = nb * (bs + (10 if trimmed else 11))
    assert (top // nb - 4) // 3 * 3 - bs == 6             # two steady triples in the longest ascending block
    return list(range(1, top + 1)) + [1, 1, 7, 1] + [1041], top
