"""Estimate a back-off n-gram over the units and write it as an ARPA file for `AVSR(ctc_ngram_lm=...)`.

    python tools/train_ngram.py UNIT_FILE (LABELS_RECORD | TEXT_FILE) ORDER OUT.arpa

The label sequences come through the pipelines avsr.LM trains on: a labels TFRecord, or a text file with one sentence per line split
into characters (symbols that are no unit are left out).  The estimator is ngram.estimate: interpolated Witten-Bell in back-off form.
Which of the two the second argument is, its first record decides (a TFRecord frame whose length checksum holds).

    python tools/train_ngram.py --words TEXT_FILE ORDER OUT.arpa

The word-level form for `AVSR(ctc_word_ngram_lm=...)`: every line of the text file is a sentence, split on spaces into words; the
same estimator runs over the word vocabulary (<s>, </s>, <unk> -- never seen, so it holds the share Witten-Bell leaves to an unseen
word -- and every word of the text) and the result is written with ngram.write_word_arpa."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _is_tfrecord(path):
    from avsr_tf1_amd.io_utils import read_tfrecord
    try:
        next(read_tfrecord(path, verify_crc=True))
        return True
    except (IOError, StopIteration, MemoryError, OverflowError):
        return False


def words_main(argv):
    from avsr_tf1_amd import ngram
    source, order, out = argv
    with open(source, "r", encoding="utf-8") as f:
        sentences = [line.split() for line in f if line.split()]
    reserved = {ngram.WORD_BOS, ngram.WORD_EOS} | set(ngram.WORD_UNK)
    vocabulary = [ngram.WORD_BOS, ngram.WORD_EOS] + sorted({w for s in sentences for w in s if w not in reserved} | {ngram.WORD_UNK[0]})
    ids = {w: i for i, w in enumerate(vocabulary)}
    unk = ids[ngram.WORD_UNK[0]]
    model = ngram.estimate([[ids.get(w, unk) for w in s] for s in sentences], int(order), ngram.word_dict(vocabulary))
    ngram.write_word_arpa(out, model, vocabulary)
    t = ngram.compile_tables(model, len(vocabulary), 0, 1)
    print("%d sentences, %d words, order %d: %s n-grams; word automaton of %d nodes, %d arcs -> %s"
          % (len(sentences), len(vocabulary) - 3, model.order, " + ".join(str(len(g)) for g in model.grams), t["n_nodes"], t["n_arcs"], out))
    return 0


def main(argv):
    if len(argv) == 4 and argv[0] == "--words":
        return words_main(argv[1:])
    if len(argv) != 4:
        print(__doc__)
        return 2
    from avsr_tf1_amd import ngram
    from avsr_tf1_amd.io_utils import create_unit_dict
    unit_file, source, order, out = argv
    ud = create_unit_dict(unit_file=unit_file)
    kw = dict(label_record=source) if _is_tfrecord(source) else dict(text_dataset=source)
    seqs = list(ngram.label_sequences(ud, **kw))
    model = ngram.estimate(seqs, int(order), ud)
    ngram.write_arpa(out, model, ud)
    t = ngram.compile_tables(model, len(ud) - 1, max(ud), max(ud) - 1)
    print("%d sequences, order %d: %s n-grams; automaton of %d nodes, %d arcs -> %s"
          % (len(seqs), model.order, " + ".join(str(len(g)) for g in model.grams), t["n_nodes"], t["n_arcs"], out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
