"""The yardstick of the time stamps and confidences of decoded hypotheses (eesen_ctc_decode_stamps, eesen_word_confidence;
INTEGRATION.md "Time stamps and CTM"), stated directly in numpy.

A best path is a vector `pos` of lattice positions per frame over L' = 2U+1 positions (odd position 2u+1 = label u, even = blank):

  label u:  lstart[u] = first frame t with pos_t == 2u+1,  lend[u] = one past the last such frame;  blank frames belong to no label
  a word is a run of labels [a, b] with an id:  wstart = lstart[a],  wend = lend[b]  (blanks inside the run are inside the interval)
    plain / token LM:   every label is its own word, the id is the class id
    spaced lexicon:     the runs between the space labels, ids in order (the space's frames belong to no word)
    unspaced lexicon:   word j covers labels [ends[j-1], ends[j] - 1], ends counted in labels
  confidence, fp64, with c = conf_scale over the n returned entries of an utterance with totals z:
    P_i = exp(c (z_i - z_0)) / sum_k exp(c (z_k - z_0))
    conf(word j of entry i, id w, [b, e)) = sum_k P_k [entry k has a word with id w whose interval intersects [b, e)]
  each entry counting at most once.
"""
import numpy as np

NONE = -1
BEYOND = -1e30


def label_intervals(pos, U, T=None):
    """(lstart, lend) [T] int32 of a path `pos` ([n] lattice positions, or all -1: no path) over U labels; -1 beyond the labels."""
    pos = np.asarray(pos, np.int64)
    T = pos.size if T is None else T
    ls, le = np.full(T, NONE, np.int32), np.full(T, NONE, np.int32)
    for u in range(U):
        at = np.flatnonzero(pos == 2 * u + 1)
        if at.size:
            ls[u], le[u] = at[0], at[-1] + 1
    return ls, le


def words_plain(labels):
    """[(id, a, b)]: every label is its own word."""
    return [(int(c), u, u) for u, c in enumerate(labels)]


def words_spaced(labels, space, ids):
    """[(id, a, b)]: the runs between the space labels carry `ids` in order."""
    runs, first = [], 0
    for u in range(len(labels) + 1):
        if u == len(labels) or labels[u] == space:
            if u > first:
                runs.append((first, u - 1))
            first = u + 1
    assert len(runs) == len(ids), (labels, space, ids)
    return [(int(w), a, b) for w, (a, b) in zip(ids, runs)]


def words_unspaced(ids, ends):
    """[(id, a, b)]: word j ends with label ends[j] - 1 and starts behind word j - 1."""
    out, first = [], 0
    for w, e in zip(ids, ends):
        out.append((int(w), first, int(e) - 1))
        first = int(e)
    return out


def word_intervals(words, ls, le):
    """[(id, wstart, wend)] of [(id, a, b)] over the label intervals."""
    return [(w, int(ls[a]), int(le[b])) for w, a, b in words]


def confidence(scores, entries, conf_scale=1.0):
    """entries[i]: [(id, wstart, wend)] of returned entry i with total scores[i].  Returns conf[i][j] in fp64."""
    z = np.asarray(scores, np.float64)
    if z.size == 0:
        return []
    p = np.exp(np.float64(conf_scale) * (z - z[0]))
    p = p / p.sum()
    out = []
    for words in entries:
        row = []
        for w, b, e in words:
            c = np.float64(0)
            for k, other in enumerate(entries):
                if any(w2 == w and b2 < e and b < e2 for w2, b2, e2 in other):
                    c += p[k]
            row.append(float(c))
        out.append(row)
    return out


def pack(entries, stride):
    """(word_len [n], ids, wstart, wend [n, stride]) int32 of entries (None: not an entry), -1 padded: eesen_word_confidence's inputs."""
    n = len(entries)
    wl = np.full(n, -1, np.int32)
    ids, b, e = (np.full((n, stride), -1, np.int32) for _ in range(3))
    for i, words in enumerate(entries):
        if words is None:
            continue
        wl[i] = len(words)
        for j, (w, b0, e0) in enumerate(words):
            ids[i, j], b[i, j], e[i, j] = w, b0, e0
    return wl, ids, b, e
