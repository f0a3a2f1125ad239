/*
 * avdsp_shard_cut.h -- where dspRuntimeSetShard cuts a chain core whose chains form memory-word trees ("shard_trees").
 * Plain C, no allocation, nothing of the runtime: avdsp_host.c includes it, and so does the stand-alone driver of
 * tests/test_shard_trees_layout.py.  avdsp_amd/sharding.py tree_shard_bounds() is the same rule in Python.
 *
 * tree_of[i] is the tree of chain i: chains with the same value belong together and must land on one rank (a trunk and the branches of
 * its word); a chain that belongs to nobody has a value of its own.  Values lie in [0, n) -- the host uses the trunk's chain index for
 * a tree and the chain's own index for every other chain.
 *
 * A position p, 0 < p < n, is OPEN if no tree has a member below p and a member at or above p (trees need not be adjacent: a tree
 * closes everything between its first and its last chain); 0 and n are always open.  Rank k's lower boundary is the open position
 * nearest to the balanced cut's, shard_range(n, world, k) -- a tie goes to the lower position --, its upper boundary is rank k + 1's
 * lower one (n for the last rank).  The balanced cuts rise with k, so the boundaries do: the ranks' ranges are disjoint, contiguous and
 * cover [0, n); a rank may come out empty.  Without trees every position is open and the result is shard_range itself.
 */
#ifndef AVDSP_SHARD_CUT_H_
#define AVDSP_SHARD_CUT_H_

/* the balanced contiguous cut: the first (total % world) ranks take one chain more (avdsp_amd/sharding.py shard_range()) */
static inline void avdsp_shard_range(int total, int world, int rank, int *lo, int *hi)
{
    const int q = total / world, r = total % world;
    *lo = rank * q + (rank < r ? rank : r);
    *hi = *lo + q + (rank < r ? 1 : 0);
}

/* bounds[0 .. world]: rank k runs chains [bounds[k], bounds[k + 1]).  scratch: 2 * n + 1 ints.  tree_of values outside [0, n) count as
 * trees of one chain. */
static inline void avdsp_tree_shard_bounds(const int *tree_of, int n, int world, int *bounds, int *scratch)
{
    int *last = scratch, *closed = scratch + n;               /* last[t]: the tree's latest chain so far; closed[p]: position p is inside a tree */
    for (int i = 0; i < n; i++) last[i] = -1;
    for (int p = 0; p <= n; p++) closed[p] = 0;
    /* a tree's members come in rising order: each one closes the positions between the member before it and itself */
    for (int i = 0; i < n; i++) {
        const int t = tree_of[i];
        if (t < 0 || t >= n) continue;
        for (int p = last[t] < 0 ? i + 1 : last[t] + 1; p <= i; p++) closed[p] = 1;
        last[t] = i;
    }
    for (int k = 0; k <= world; k++) {
        int want, hi_;
        if (k == world) { bounds[k] = n; break; }
        avdsp_shard_range(n, world, k, &want, &hi_);
        int best = 0;
        for (int d = 0; d <= n; d++) {                         /* the lower position first: it wins a tie */
            if (want - d >= 0 && !closed[want - d]) { best = want - d; break; }
            if (want + d <= n && !closed[want + d]) { best = want + d; break; }
        }
        bounds[k] = best;
    }
}

#endif
