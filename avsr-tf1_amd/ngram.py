"""Back-off n-gram language models over the unit vocabulary, host side (numpy only; importable without a GPU): the ARPA text format in
and out, a small estimator, and the compiler of the device automaton that the CTC prefix beam search walks inside its frame loop
(csrc/ctc_prefix_ngram.hip) and beam search walks once per decode step (csrc/beam_ngram.hip); the rules are INTEGRATION.md section 8.

The model of order N over the classes 0 .. V-1 (MASK = 0, the units, EOS = V-2, GO = V-1 -- io_utils.create_unit_dict):
    context   h = the last N-1 symbols of (GO, g_0 .. g_{n-1}); empty for N = 1
    back-off  lam(c | h) = the listed value of h.c, else bow(h) + lam(c | h[1:]) with bow(h) = 0 for an unlisted h
    floor     an unlisted class at the empty context gets FLOOR = -99 ln 10 (ARPA's "impossible", finite on purpose)
`NGramModel` keeps ARPA's own numbers (log10, float64), so writing and reading a file gives the identical model; natural logs are formed
in float64 where they are used and rounded to float32 once, in `compile_tables`.

Tokens: <s> is GO, </s> is EOS, <space> is the unit ' ', every other token is the unit's own string (multi-character units work).
Entries that contain <unk> are DROPPED and their probability mass is not given to anything else: the recogniser has no unknown unit."""
import math

import numpy as np

LN10 = math.log(10.0)
FLOOR = -99.0 * LN10
MAX_ORDER = 16                         # AVSR_CTC_PREFIX_NGRAM_MAX_ORDER of include/avsr_hip.h: the device walk visits at most 15 nodes


class NGramModel:
    """order N and grams[k - 1] = {k-gram as a tuple of class ids: (log10 p, log10 bow)}, bow 0.0 where the file has no column."""

    def __init__(self, order, grams):
        self.order, self.grams = int(order), [dict(g) for g in grams]
        if self.order < 1 or len(self.grams) != self.order:
            raise ValueError("an n-gram model needs one table per order 1 .. N (got order %r, %d tables)" % (order, len(grams)))

    def __eq__(self, other):
        return isinstance(other, NGramModel) and self.order == other.order and self.grams == other.grams

    def __repr__(self):
        return "NGramModel(order=%d, counts=%r)" % (self.order, [len(g) for g in self.grams])


def _tokens(unit_dict):
    """class id -> ARPA token, for the classes that have one (MASK and END have none)."""
    out = {}
    for i, s in unit_dict.items():
        if s in ("MASK", "END"):
            continue
        out[i] = {"GO": "<s>", "EOS": "</s>", " ": "<space>"}.get(s, s)
    return out


def read_arpa(path, unit_dict):
    """Parse an ARPA file into an NGramModel over unit_dict's classes (id -> symbol, io_utils.create_unit_dict).  ValueError for a file
    without a \\1-grams: section, a malformed line, a count that contradicts the \\data\\ header, or a token that is not a unit."""
    ids = {t: i for i, t in _tokens(unit_dict).items()}
    counts, grams, k, seen = {}, {}, 0, {}
    in_data = False
    with open(path, "r", encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if line == "\\data\\":
                in_data = True
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                try:
                    k = int(line[1:-len("-grams:")])
                except ValueError:
                    raise ValueError("%s:%d: not a section header: %r" % (path, ln, line))
                in_data = False
                grams.setdefault(k, {})
                seen.setdefault(k, 0)
                continue
            if in_data:
                if line.startswith("ngram ") and "=" in line:
                    a, b = line[len("ngram "):].split("=", 1)
                    counts[int(a)] = int(b)
                continue
            if k == 0:
                continue                                   # (text before \data\)
            f_ = line.split()
            if len(f_) not in (k + 1, k + 2):
                raise ValueError("%s:%d: a %d-gram line has %d or %d fields: %r" % (path, ln, k, k + 1, k + 2, line))
            try:
                lp, bow = float(f_[0]), float(f_[k + 1]) if len(f_) == k + 2 else 0.0
            except ValueError:
                raise ValueError("%s:%d: not a number in %r" % (path, ln, line))
            seen[k] += 1
            toks = f_[1:k + 1]
            if "<unk>" in toks or "<UNK>" in toks:
                continue                                   # dropped; the lost mass is not renormalised
            for t in toks:
                if t not in ids:
                    raise ValueError("%s:%d: token %r is not a unit of the unit file" % (path, ln, t))
            grams[k][tuple(ids[t] for t in toks)] = (lp, bow)
    if 1 not in grams:
        raise ValueError("%s: no \\1-grams: section -- not an ARPA language model" % path)
    order = max(grams)
    for j in range(1, order + 1):
        if j not in grams:
            raise ValueError("%s: no \\%d-grams: section below the \\%d-grams: one" % (path, j, order))
        if j in counts and counts[j] != seen[j]:
            raise ValueError("%s: the header announces %d %d-grams, the section holds %d" % (path, counts[j], j, seen[j]))
    return NGramModel(order, [grams[j] for j in range(1, order + 1)])


def write_arpa(path, model, unit_dict):
    """Write the model with repr()'s digits (read_arpa gives the identical model back); orders below N carry the back-off column."""
    tok = _tokens(unit_dict)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, g in enumerate(model.grams, 1):
            f.write("ngram %d=%d\n" % (k, len(g)))
        for k, g in enumerate(model.grams, 1):
            f.write("\n\\%d-grams:\n" % k)
            for gram in sorted(g):
                lp, bow = g[gram]
                words = " ".join(tok[i] for i in gram)
                if k < model.order or bow != 0.0:
                    f.write("%r\t%s\t%r\n" % (float(lp), words, float(bow)))
                else:
                    f.write("%r\t%s\n" % (float(lp), words))
        f.write("\n\\end\\\n")


def estimate(sequences, order, unit_dict):
    """Interpolated Witten-Bell over the events GO g_0 .. g_{n-1} EOS of every label sequence, written in back-off form:
        p(c | h) = (n(hc) + T(h) p(c | h[1:])) / (n(h) + T(h))     T(h) = the number of distinct classes seen after h
        bow(h)   = T(h) / (n(h) + T(h))
    with the order-0 base uniform over the real units plus EOS.  Every real unit and EOS is a listed unigram, GO is the unigram -99 with
    its back-off weight, and a k-gram is listed where it was seen.  Sequences hold class ids of real units only."""
    order = int(order)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError("the n-gram order must lie in 1 .. %d (got %d)" % (MAX_ORDER, order))
    rev = {s: i for i, s in unit_dict.items()}
    go, eos = rev["GO"], rev["EOS"]
    real = sorted(i for i, s in unit_dict.items() if s not in ("MASK", "END", "GO", "EOS"))
    cnt = [dict() for _ in range(order)]                       # cnt[k - 1][h][c] = n(hc), h of length k - 1
    for g in sequences:
        g = [int(s) for s in g]
        for s in g:
            if s not in real:
                raise ValueError("a label sequence holds class %d, which is no real unit" % s)
        ev = [go] + g + [eos]
        for i in range(1, len(ev)):
            for k in range(1, order + 1):
                if i - k + 1 < 0:
                    break
                h = tuple(ev[i - k + 1:i])
                d = cnt[k - 1].setdefault(h, {})
                d[ev[i]] = d.get(ev[i], 0) + 1
    base = 1.0 / (len(real) + 1)
    prob = [dict() for _ in range(order)]                      # prob[k - 1][h + (c,)] = p(c | h), natural scale
    bows = {}

    def lower(h, c):                                           # p(c | h) in back-off form, h of any length < order
        if h + (c,) in prob[len(h)]:
            return prob[len(h)][h + (c,)]
        if not h:
            return 0.0
        return bows.get(h, 1.0) * lower(h[1:], c)

    uni = cnt[0].get((), {})
    n0, t0 = sum(uni.values()), len(uni)
    for c in real + [eos]:
        prob[0][(c,)] = (uni.get(c, 0) + t0 * base) / (n0 + t0) if n0 else base
    for k in range(2, order + 1):
        for h, d in cnt[k - 1].items():
            n, t = sum(d.values()), len(d)
            bows[h] = t / (n + t)
            for c, m in d.items():
                prob[k - 1][h + (c,)] = (m + t * lower(h[1:], c)) / (n + t)
    grams = [dict() for _ in range(order)]
    for k in range(1, order + 1):
        for gram, p in prob[k - 1].items():
            grams[k - 1][gram] = (math.log(p) / LN10, math.log(bows[gram]) / LN10 if k < order and gram in bows else 0.0)
    grams[0][(go,)] = (-99.0, math.log(bows[(go,)]) / LN10 if (go,) in bows else 0.0)
    return NGramModel(order, grams)


def compile_tables(model, V, go_id, eos_id):
    """The device automaton of include/avsr_hip.h avsr_ctc_prefix_ngram as numpy arrays:
        dict(order, V, go_id, eos_id, start, n_nodes, n_arcs, bow f32 [n_nodes], backoff i32 [n_nodes], arc_begin i32 [n_nodes + 1],
             sym i32 [n_arcs], logp f32 [n_arcs], next i32 [n_arcs], contexts = the nodes' contexts as tuples (host only))
    Node 0 is the root and holds one arc per class 0 .. V-1 (FLOOR and next = root for a class the model lacks).  Every other node is a
    listed n-gram of order 1 .. N-1, or a context that only appears inside higher-order entries (bow 0), or a prefix of such a node.
    A node whose own n-gram h.c is not listed would be unreachable -- the walk finds it through the arc c of h -- so that arc is added
    with the value the back-off rule gives it anyway, bow(h) + lam(c | h[1:]) formed in float64: the model's values do not change."""
    V, go_id, eos_id = int(V), int(go_id), int(eos_id)
    N = model.order
    if N > MAX_ORDER:
        raise ValueError("n-gram orders of up to %d are supported (got %d)" % (MAX_ORDER, N))
    if not (0 <= go_id < V and 0 <= eos_id < V):
        raise ValueError("GO and EOS must be classes below V = %d (got %d, %d)" % (V, go_id, eos_id))
    lp, bw = {}, {}
    for k, g in enumerate(model.grams, 1):
        for gram, (a, b) in g.items():
            if len(gram) != k or any(not 0 <= c < V for c in gram):
                raise ValueError("the %d-gram %r does not fit %d classes" % (k, gram, V))
            lp[gram], bw[gram] = a * LN10, b * LN10

    def lam(c, h):                                             # the textbook rule, float64
        if h + (c,) in lp:
            return lp[h + (c,)]
        if not h:
            return FLOOR
        return bw.get(h, 0.0) + lam(c, h[1:])

    nodes = {()}
    for gram in lp:
        for h in ((gram,) if len(gram) < N else ()) + (gram[:-1],):
            while h and h not in nodes:                        # ... and its prefixes
                nodes.add(h)
                h = h[:-1]
    for h in sorted(nodes, key=lambda h: (len(h), h)):         # shorter first: a completed entry never changes a value below it
        if h and h not in lp:
            lp[h] = lam(h[-1], h[:-1])
    order = sorted(nodes, key=lambda h: (len(h), h))
    index = {h: i for i, h in enumerate(order)}

    def suffix_node(h):                                        # the longest suffix of h that is a node
        h = h[max(len(h) - (N - 1), 0):] if N > 1 else ()
        while h not in index:
            h = h[1:]
        return index[h]

    arcs = {h: [] for h in order}
    for gram in lp:
        if gram[:-1] in arcs:
            arcs[gram[:-1]].append(gram[-1])
    bow, backoff, arc_begin, sym, logp, nxt = [], [], [0], [], [], []
    for h in order:
        bow.append(bw.get(h, 0.0) if h else 0.0)
        backoff.append(suffix_node(h[1:]) if h else 0)
        for c in (range(V) if not h else sorted(arcs[h])):
            sym.append(c)
            logp.append(lp.get(h + (c,), FLOOR))
            nxt.append(suffix_node(h + (c,)) if h + (c,) in lp else 0)
        arc_begin.append(len(sym))
    return dict(order=N, V=V, go_id=go_id, eos_id=eos_id, start=index.get((go_id,), 0), n_nodes=len(order), n_arcs=len(sym),
                bow=np.asarray(bow, np.float64).astype(np.float32), backoff=np.asarray(backoff, np.int32),
                arc_begin=np.asarray(arc_begin, np.int32), sym=np.asarray(sym, np.int32),
                logp=np.asarray(logp, np.float64).astype(np.float32), next=np.asarray(nxt, np.int32), contexts=order)


def walk(tables, node, c):
    """The device walk restated in numpy float32, additions in the kernel's order: (lam(c | node's context), the arc it ended on)."""
    acc = np.float32(0.0)
    ab, sy = tables["arc_begin"], tables["sym"]
    while node != 0:
        lo, hi = int(ab[node]), int(ab[node + 1])
        a = lo + int(np.searchsorted(sy[lo:hi], c))
        if a < hi and sy[a] == c:
            return np.float32(acc + tables["logp"][a]), a
        acc = np.float32(acc + tables["bow"][node])
        node = int(tables["backoff"][node])
    return np.float32(acc + tables["logp"][c]), int(c)


def load_tables(path, unit_dict):
    """read_arpa + compile_tables over unit_dict's classes."""
    rev = {s: i for i, s in unit_dict.items()}
    return compile_tables(read_arpa(path, unit_dict), len(unit_dict) - 1, rev["GO"], rev["EOS"])


def label_sequences(unit_dict, label_record=None, text_dataset=None):
    """The label sequences of a labels TFRecord or of a text file (one sentence per line), through the pipelines avsr.LM trains on:
    the record's trailing EOS is taken off again, symbols that are no unit are left out."""
    from .io_utils import make_iterator_from_label_record, make_iterator_from_text_dataset
    rev = {s: i for i, s in unit_dict.items()}
    real = {i for i, s in unit_dict.items() if s not in ("MASK", "END", "GO", "EOS")}
    pipe = (make_iterator_from_label_record(label_record, 1, unit_dict) if text_dataset is None
            else make_iterator_from_text_dataset(text_dataset, 1, unit_dict))
    for _inp, (ids, n, _name) in pipe._examples():
        ids = [int(s) for s in np.asarray(ids).reshape(-1)[:int(n)]]
        if ids and ids[-1] == rev["EOS"]:
            ids = ids[:-1]
        yield [s for s in ids if s in real]
