"""The fixed-order float64 sum of csrc/fixed_sum.inc, restated in numpy: which additions are made, and in which order.

A grid of `blocks` blocks of `threads` threads sums n items of c float64 components each.  Thread t of block b adds the items
b * threads + t + m * blocks * threads in rising m, and the components of an item in their order, from 0.0.  The values of a block
go through the halving tree (slot t < h takes slot t + h for h = threads / 2 .. 1), and the blocks are added in their order, from 0.0.
Every operation is one IEEE float64 addition, so the result is the kernels' bit for bit wherever the terms are."""
import numpy as np


def grid_sum(terms, blocks, threads=256):
    """`terms`: [n] or [n, c] float64.  The sum of all of them in the order of the reduce grid, as a Python float."""
    terms = np.asarray(terms, dtype=np.float64)
    terms = terms.reshape(len(terms), -1)
    sweep = blocks * threads
    sweeps = -(-len(terms) // sweep)
    padded = np.zeros((sweeps * sweep, terms.shape[1]))  # x + (+0.0) == x for every x a sum from +0.0 can reach
    padded[:len(terms)] = terms
    acc = np.zeros((blocks, threads))
    for plane in padded.reshape(sweeps, blocks, threads, -1):
        for c in range(plane.shape[-1]):
            acc += plane[..., c]
    h = threads // 2
    while h:
        acc[:, :h] += acc[:, h:2 * h]
        h //= 2
    total = 0.0
    for partial in acc[:, 0]:  # not np.sum: that one adds pairwise
        total += float(partial)
    return total


def grid_sum_by_thread(terms, blocks, threads=256):
    """The same sum, thread by thread and addition by addition: what grid_sum is checked against."""
    terms = np.asarray(terms, dtype=np.float64)
    terms = terms.reshape(len(terms), -1).tolist()
    total = 0.0
    for b in range(blocks):
        slots = []
        for t in range(threads):
            s = 0.0
            for i in range(b * threads + t, len(terms), blocks * threads):
                for v in terms[i]:
                    s += v
            slots.append(s)
        h = threads // 2
        while h:
            for t in range(h):
                slots[t] += slots[t + h]
            h //= 2
        total += slots[0]
    return total
