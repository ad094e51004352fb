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
Entries that contain <unk> are DROPPED and their probability mass is not given to anything else: the recogniser has no unknown unit.

The second half of the file is the WORD-level form for models over single-character units (csrc/ctc_prefix_word_ngram.hip): ARPA files
whose tokens are words (`read_word_arpa`, `write_word_arpa`; <unk> is kept there), `compile_word_tables` -- the same automaton over word
ids plus a trie over the words' spellings -- and `word_step` / `word_lam`, the kernel's step restated in numpy float32."""
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


def _parse_arpa(path, gram_of):
    """The ARPA text of `path` as (order, [{gram_of(tokens): (log10 p, log10 bow)} per order]); gram_of(tokens, where) gives an entry's
    key, None to drop the entry, or raises ValueError for a token it does not know (where = "path:line").  ValueError for a file
    without a \\1-grams: section, a malformed line or a count that contradicts the \\data\\ header."""
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
                continue                                   # (text before \\data\\)
            f_ = line.split()
            if len(f_) not in (k + 1, k + 2):
                raise ValueError("%s:%d: a %d-gram line has %d or %d fields: %r" % (path, ln, k, k + 1, k + 2, line))
            try:
                lp, bow = float(f_[0]), float(f_[k + 1]) if len(f_) == k + 2 else 0.0
            except ValueError:
                raise ValueError("%s:%d: not a number in %r" % (path, ln, line))
            seen[k] += 1
            gram = gram_of(f_[1:k + 1], "%s:%d" % (path, ln))
            if gram is not None:
                grams[k][gram] = (lp, bow)
    if 1 not in grams:
        raise ValueError("%s: no \\1-grams: section -- not an ARPA language model" % path)
    order = max(grams)
    for j in range(1, order + 1):
        if j not in grams:
            raise ValueError("%s: no \\%d-grams: section below the \\%d-grams: one" % (path, j, order))
        if j in counts and counts[j] != seen[j]:
            raise ValueError("%s: the header announces %d %d-grams, the section holds %d" % (path, counts[j], j, seen[j]))
    return order, [grams[j] for j in range(1, order + 1)]


def read_arpa(path, unit_dict):
    """Parse an ARPA file into an NGramModel over unit_dict's classes (id -> symbol, io_utils.create_unit_dict).  ValueError for a file
    without a \\1-grams: section, a malformed line, a count that contradicts the \\data\\ header, or a token that is not a unit."""
    ids = {t: i for i, t in _tokens(unit_dict).items()}

    def gram_of(toks, where):
        if "<unk>" in toks or "<UNK>" in toks:
            return None                                    # dropped; the lost mass is not renormalised
        for t in toks:
            if t not in ids:
                raise ValueError("%s: token %r is not a unit of the unit file" % (where, t))
        return tuple(ids[t] for t in toks)
    return NGramModel(*_parse_arpa(path, gram_of))


def write_arpa(path, model, unit_dict):
    """Write the model with repr()'s digits (read_arpa gives the identical model back); orders below N carry the back-off column."""
    _write_arpa(path, model, _tokens(unit_dict))


def _write_arpa(path, model, tok):
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


# ---- word-level models behind a lexicon trie (csrc/ctc_prefix_word_ngram.hip; the rule is INTEGRATION.md section 8) ----
# The search runs over characters; the state of a label sequence is (h, p): h the word automaton's node for the words closed so far,
# p the trie node of the letters since the last space (0 = the trie's root, WORD_OOV once they have left every spelling).

WORD_BOS, WORD_EOS, WORD_UNK = "<s>", "</s>", ("<unk>", "<UNK>")
WORD_OOV = -1


def read_word_arpa(path):
    """Parse an ARPA file whose tokens are WORDS into (NGramModel over word ids, vocabulary).  vocabulary[id] is the token: <s> is 0,
    </s> is 1, every other token of the file follows in sorted order -- <unk> / <UNK>, which is KEPT here, among them.  read_arpa's
    file errors."""
    order, grams = _parse_arpa(path, lambda toks, where: tuple(toks))
    vocabulary = [WORD_BOS, WORD_EOS] + sorted({t for g in grams for gram in g for t in gram} - {WORD_BOS, WORD_EOS})
    ids = {t: i for i, t in enumerate(vocabulary)}
    return NGramModel(order, [{tuple(ids[t] for t in gram): v for gram, v in g.items()} for g in grams]), vocabulary


def write_word_arpa(path, model, vocabulary):
    """write_arpa for a model over word ids; read_word_arpa gives the identical (model, vocabulary) back when the vocabulary is in its
    order (<s>, </s>, the rest sorted) and every word occurs in the model."""
    _write_arpa(path, model, dict(enumerate(vocabulary)))


def word_dict(vocabulary):
    """The {id: name} dictionary `estimate` takes, for a vocabulary in read_word_arpa's order: <s> as GO, </s> as EOS, every other
    word a real class (the names are tagged, so that no word reads as one of the dictionary's reserved names)."""
    if list(vocabulary[:2]) != [WORD_BOS, WORD_EOS]:
        raise ValueError("a word vocabulary starts with %s, %s (got %r)" % (WORD_BOS, WORD_EOS, list(vocabulary[:2])))
    d = {i: "w:" + w for i, w in enumerate(vocabulary)}
    d[0], d[1] = "GO", "EOS"
    return d


def compile_word_tables(model, vocabulary, unit_dict, oov_score=-10.0):
    """The device tables of include/avsr_hip.h avsr_ctc_prefix_word_ngram as numpy arrays, for a word model (read_word_arpa) decoded
    over the single-character units of unit_dict:
        the word automaton   compile_tables(model, Vw, <s>, </s>) unchanged: order, start, n_nodes, n_arcs, bow, backoff, arc_begin, sym,
                             logp, next, contexts -- with its classes under Vw, go_w, eos_w, and unk_id (-1 without <unk>)
        the lexicon trie     CSR over the spellings: t_begin i32 [n_trie_nodes + 1], t_sym i32 [n_trie_arcs] (unit ids, sorted per node),
                             t_next i32 [n_trie_arcs], t_word i32 [n_trie_nodes] (the word a node ends, or -1); node 0 is the root
        the units            V, go_id, eos_id, space_id; oov_score (natural log, <= 0); n_unspellable
    A word is spelled by its own characters.  One with a character that is no letter of the unit file (a letter: every unit but ' ')
    stays in the model as context and is left out of the trie; so are <s>, </s> and <unk>.
    ValueError: a unit file without ' ' or with a unit longer than one character, no spellable word, oov_score positive or not finite,
    an order above MAX_ORDER."""
    oov = float(oov_score)
    if not oov <= 0.0 or oov == float("-inf"):
        raise ValueError("the out-of-vocabulary score must be a finite number <= 0 (got %r)" % (oov_score,))
    rev = {s: i for i, s in unit_dict.items()}
    if " " not in rev:
        raise ValueError("a word-level n-gram needs the unit ' ' in the unit file: a space closes a word")
    letters = {}
    for i, s in unit_dict.items():
        if s in ("MASK", "END", "GO", "EOS", " "):
            continue
        if len(s) != 1:
            raise ValueError("a word-level n-gram needs single-character units: words are spelled by their characters (unit %r; phoneme "
                             "and viseme lists need a pronunciation lexicon, which is not built)" % (s,))
        letters[s] = i
    vocabulary = list(vocabulary)
    idw = {w: i for i, w in enumerate(vocabulary)}
    if len(idw) != len(vocabulary) or WORD_BOS not in idw or WORD_EOS not in idw:
        raise ValueError("a word vocabulary holds %s, %s and every word once" % (WORD_BOS, WORD_EOS))
    t = compile_tables(model, len(vocabulary), idw[WORD_BOS], idw[WORD_EOS])
    t["Vw"], t["go_w"], t["eos_w"] = t.pop("V"), t.pop("go_id"), t.pop("eos_id")
    t["unk_id"] = idw.get(WORD_UNK[0], idw.get(WORD_UNK[1], WORD_OOV))
    children, ends, unspellable = [{}], [-1], 0
    for wid, w in enumerate(vocabulary):
        if w in (WORD_BOS, WORD_EOS) + WORD_UNK:
            continue
        if not w or any(ch not in letters for ch in w):
            unspellable += 1
            continue
        n = 0
        for ch in w:
            if letters[ch] not in children[n]:
                children[n][letters[ch]] = len(children)
                children.append({})
                ends.append(-1)
            n = children[n][letters[ch]]
        ends[n] = wid
    if len(children) == 1:
        raise ValueError("no word of the model can be spelled with the letters of the unit file (%d words)" % unspellable)
    t_begin, t_sym, t_next = [0], [], []
    for ch in children:
        for c in sorted(ch):
            t_sym.append(c)
            t_next.append(ch[c])
        t_begin.append(len(t_sym))
    t.update(V=len(unit_dict) - 1, go_id=rev["GO"], eos_id=rev["EOS"], space_id=rev[" "], oov_score=oov, n_unspellable=unspellable,
             n_trie_nodes=len(children), n_trie_arcs=len(t_sym), t_begin=np.asarray(t_begin, np.int32), t_sym=np.asarray(t_sym, np.int32),
             t_next=np.asarray(t_next, np.int32), t_word=np.asarray(ends, np.int32))
    return t


def word_start(tables):
    """The state of the empty label sequence."""
    return int(tables["start"]), 0


def _trie_child(t, p, c):
    lo, hi = int(t["t_begin"][p]), int(t["t_begin"][p + 1])
    a = lo + int(np.searchsorted(t["t_sym"][lo:hi], c))
    return int(t["t_next"][a]) if a < hi and t["t_sym"][a] == c else WORD_OOV


def _word_close(t, h, p):
    """What a space costs at (h, p) and the automaton node it leaves, float32 in the kernel's order."""
    if p == 0:
        return np.float32(0.0), h
    w = int(t["t_word"][p]) if p > 0 else -1
    prefix = p > 0 and w < 0
    if w < 0:
        w = int(t["unk_id"])
    if w >= 0:
        v, arc = walk(t, h, w)
        hc = int(t["next"][arc])
    else:
        v, hc = np.float32(0.0), 0
    return (np.float32(np.float32(t["oov_score"]) + v) if prefix else v), hc


def word_step(tables, state, c):
    """The device step restated: the state of g.c from the state of g."""
    t, (h, p), c = tables, state, int(c)
    if c == t["space_id"]:
        return (_word_close(t, h, p)[1], 0) if p != 0 else (h, p)
    if c == t["eos_id"]:
        return int(t["next"][walk(t, _word_close(t, h, p)[1], t["eos_w"])[1]]), 0
    if c == t["go_id"] or c == 0:
        return h, p
    return h, (_trie_child(t, p, c) if p >= 0 else WORD_OOV)


def word_lam(tables, state):
    """The device row restated in numpy float32, additions in the kernel's order: lam(. | g) [V] at the state of g."""
    t, (h, p) = tables, state
    oov = np.float32(t["oov_score"])
    row = np.zeros(t["V"], np.float32)
    if p >= 0:
        lo, hi = int(t["t_begin"][p]), int(t["t_begin"][p + 1])
        row[:] = oov
        row[t["t_sym"][lo:hi]] = 0.0
    cl, hc = _word_close(t, h, p)
    row[t["space_id"]] = cl
    row[t["eos_id"]] = np.float32(cl + walk(t, hc, t["eos_w"])[0])
    row[t["go_id"]] = row[0] = np.float32(FLOOR)
    return row


def load_word_tables(path, unit_dict, oov_score=-10.0):
    """read_word_arpa + compile_word_tables over unit_dict's classes."""
    model, vocabulary = read_word_arpa(path)
    return compile_word_tables(model, vocabulary, unit_dict, oov_score)


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
