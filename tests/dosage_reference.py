"""Plain numpy references of the 2-bit dosage sweeps, shared by the GPU tests: counting over the codes themselves, none of
the kernels' bit tricks.  codes are [rows][genomes] uint8 in 0..3 (3 = more than two copies, "non diploid")."""
import numpy as np


def row_lists(codes, g0, g1, selected=None, keep=None):
    """kgx_genome_row_lists: for every genome of [g0, g1) the (selected) rows it carries, ascending; (begin, rows)."""
    begin, rows = [0], []
    for g in range(g0, g1):
        if keep is None or keep[g]:
            carried = np.nonzero((codes[:, g] > 0) & (selected if selected is not None else True))[0]
            rows.extend(carried.tolist())
        begin.append(len(rows))
    return np.array(begin, dtype=np.uint64), np.array(rows, dtype=np.uint32)


def counts_by_code(codes, axis):
    """How often each of the four codes occurs along `axis`: [...][4]."""
    return np.stack([(codes == k).sum(axis) for k in range(4)], -1)


def compound_offsets(codes, groups, n_bins):
    """kgx_compound_offsets as kgx.h states it.  groups: (rows of the group, bin).  A genome with n copies at the offset (code 3
    counting as three or more): n == 1 -> heterozygous_reference_minor += 1; n >= 2 -> homozygous_minor += distinct variants
    carried, heterozygous_minor += variants carried exactly once.  [genomes][n_bins][3] uint64."""
    out = np.zeros((codes.shape[1], n_bins, 3), dtype=np.uint64)
    for rows, b in groups:
        block = codes[rows].astype(np.int64)
        copies = block.sum(0)                                    # code 3 = "three or more": any such cell makes n >= 2
        carried = (block > 0).sum(0)
        once = (block == 1).sum(0)
        out[:, b, 0] += (copies == 1).astype(np.uint64)
        out[:, b, 1] += np.where(copies >= 2, carried, 0).astype(np.uint64)
        out[:, b, 2] += np.where(copies >= 2, once, 0).astype(np.uint64)
    return out


def offset_filter_counts(codes, offsets, n_bins):
    """kgx_offset_filter_counts as kgx.h states it.  offsets: (rows of the offset -- one or more --, bin).  At an offset a
    genome holds ns variants once, n2 twice, n3 more often: HomozygousFilter leaves 2 objects iff n3 == 0, n2 == 1, ns == 0;
    HeterozygousFilter ns; DiploidFilter ns + 2 n2 iff n3 == 0 and that is at most 2; UniqueUnphasedFilter ns + n2 + n3.
    [genomes][n_bins][4] uint64."""
    out = np.zeros((codes.shape[1], n_bins, 4), dtype=np.uint64)
    for rows, b in offsets:
        block = codes[rows]
        ns, n2, n3 = (block == 1).sum(0), (block == 2).sum(0), (block == 3).sum(0)
        objects = ns + 2 * n2
        out[:, b, 0] += np.where((n3 == 0) & (n2 == 1) & (ns == 0), 2, 0).astype(np.uint64)
        out[:, b, 1] += ns.astype(np.uint64)
        out[:, b, 2] += np.where((n3 == 0) & (objects <= 2), objects, 0).astype(np.uint64)
        out[:, b, 3] += (ns + n2 + n3).astype(np.uint64)
    return out
