"""A Python model of the cost-minimising parse against a prepared dictionary
(APE_LZ4_hc_cdict_prepare_dev + APE_LZ4_compress_hc_opt_usingCDict_batch_dev).
No new policy: the block of message m is hcoptmodel.compress_prefix() on hcdictmodel.window()'s
window [the dictionary's last D bytes | m].  This file holds that call, the searched window the
tests price more than once, and one handle for the wrong neighbour that only this kernel can
have.  No product or oracle code."""
import functools

import hcdictmodel
import hclargemodel
import hcoptmodel
from hcmodel import CAP, LASTLITERALS


@functools.lru_cache(maxsize=64)   # (a window's lists take about a megabyte)
def searched(dictionary, message, max_src_size, depth):
    """(window, D, ML, MQ): the window of `message` and the search's matches over it (lists by
    window position; hclargemodel.search is hcdictmodel's search too)."""
    assert len(message) <= max_src_size
    D = hcdictmodel.window(len(dictionary), max_src_size)
    win = bytes(dictionary[len(dictionary) - D:]) + bytes(message)
    ML, MQ = hclargemodel.search(win, D, depth)
    return win, D, ML.tolist(), MQ.tolist()


def full_length_stop_at_dict(D):
    """The wrong neighbour's E(p): a capped match whose source lies in the dictionary is
    extended no further than the dictionary's end (it keeps what the search reported)."""
    def full_length(window, prefix, ML, MQ):
        E = hcoptmodel.full_length_plain(window, prefix, ML, MQ)
        W = len(window)
        for p, L in enumerate(ML):
            if L == CAP and W - LASTLITERALS - p > CAP and MQ[p] < D:
                E[p] = max(L, min(E[p], D - MQ[p]))
        return E
    return full_length


def compress(dictionary, message, max_src_size, depth, rule=hcoptmodel.RULE, stop_at_dict=False):
    """The block the GPU writes for `message` (at most max_src_size bytes) against an object
    prepared from `dictionary` for max_src_size; it decodes with decompress_safe_usingDict given
    the whole dictionary.  stop_at_dict moves it to the wrong neighbour."""
    win, D, ML, MQ = searched(bytes(dictionary), bytes(message), max_src_size, depth)
    if not stop_at_dict:
        return hcoptmodel.parse_opt(win, D, ML, MQ, rule)
    # (the neighbour's E replaces the model's for this one walk: a shorter E is still a match's
    # length, so the walk stays a valid block and A[D] its size)
    keep = hcoptmodel.full_length
    hcoptmodel.full_length = full_length_stop_at_dict(D)
    try:
        return hcoptmodel.parse_opt(win, D, ML, MQ, rule)
    finally:
        hcoptmodel.full_length = keep

