"""TEST INFRASTRUCTURE: the tag facets by their definition, in numpy - what every facets test expects.  Given the tags of the match set A
(from the oracle's match set, never from the library's output) and the scope, the 34 words of include/frizbee_hip.h's layout."""
import numpy as np

WORDS, BITS = 34, 16


def visible(tags, require, exclude):
    t = np.asarray(tags, np.uint32)
    return ((t & require) == require) & ((t & exclude) == 0)


def facet_words(tags_of_a, require=0, exclude=0):
    t = np.asarray(tags_of_a, np.uint32)
    vis = visible(t, require, exclude)
    out = np.zeros(WORDS, np.uint32)
    out[0] = len(t)
    out[1] = int(vis.sum())
    for b in range(BITS):
        has = ((t >> b) & 1).astype(bool)
        out[2 + b] = int(has.sum())
        out[2 + BITS + b] = int((has & vis).sum())
    return out


def as_dict(words):
    return dict(matched=int(words[0]), visible=int(words[1]), all_by_bit=[int(x) for x in words[2:2 + BITS]], visible_by_bit=[int(x) for x in words[2 + BITS:2 + 2 * BITS]])
