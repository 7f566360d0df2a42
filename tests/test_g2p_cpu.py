"""CPU: the host side of the grapheme-to-phoneme model (fastspeech2_amd/g2p.py) and the reference the GPU tests lean on."""
import json
import math
import os
import types

import numpy as np
import pytest

from fastspeech2_amd import g2p
from tests import g2p_corpus, g2p_ref

A, P = 6, 8
BARS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2p_bars.json")


@pytest.fixture(scope="module")
def small():
    lex = g2p_corpus.lexicon(1, 140)
    entries, letters, phones = g2p_corpus.ids(lex)
    m = g2p_ref.train_model(entries[:120], A, P, order=4, iters=2)
    return m, entries, letters, phones


def test_reference_beam_search_equals_brute_force_on_short_words(small):
    m, _, _, _ = small
    T = len(m["tokens"])
    words = [[a] for a in range(A)] + [[a, b] for a in range(A) for b in range(A)] + \
            [[a, b, c] for a in range(A) for b in range(A) for c in range(A)]
    decided = 0
    for w in words:                                                        # every word of at most 3 letters, ties included
        brute, score, n_paths = g2p_ref.brute_force(w, m["spelling"], m["model"], 4, T, m["type_phones"])
        got, got_score, _, _ = g2p_ref.beam_search(w, m["spelling"], m["model"], 4, max(n_paths, 1), T, m["type_phones"])
        assert got_score == score and got == brute, w
        decided += brute is not None
    assert decided > len(words) // 2


def test_every_context_sums_to_one_through_the_back_off_form(small):
    m, _, _, _ = small
    T = len(m["tokens"])
    for N in (1, 2, 4):
        lm = g2p.kneser_ney(m["seqs"], T, N)
        md = g2p_ref.model_from_arrays(lm, N)
        ref, _ = g2p_ref.kneser_ney(m["seqs"], T, N)
        for n in range(1, N + 1):                                         # the product's estimate is the reference's
            assert set(md[n]) == set(ref[n])
            for key, (lp, bow) in md[n].items():
                assert bow == pytest.approx(ref[n][key][1], abs=1e-12)
                assert lp == ref[n][key][0] or lp == pytest.approx(ref[n][key][0], abs=1e-12)
        contexts = {()} if N == 1 else {(T,) * (N - 1)}
        for n in range(2, N + 1):
            contexts |= {(T,) * (N - n) + key[:-1] for key in md[n]}
        for h in contexts | {tuple([0] * (N - 1))}:
            total = sum(math.exp(g2p_ref.lookup(md, N, h, w)) for w in list(range(T)) + [T + 1])
            assert abs(total - 1.0) <= 1e-12, (N, h, total)


def test_npz_round_trip_is_exact_and_needs_no_pickle(small, tmp_path):
    m, _, letters, phones = small
    lm = g2p.kneser_ney(m["seqs"], len(m["tokens"]), 4)
    summary = {"entries_used": 120, "skipped": {"limit": 0, "empty": 1, "no_path": 2}, "loglik": [-3.5, -2.25]}
    model = g2p.G2P(letters, phones, m["type_letters"], m["type_phones"], lm, 4, 64, summary)
    path = str(tmp_path / "model.npz")
    model.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    back = g2p.G2P.load(path)
    assert back.letters == model.letters and back.phones == model.phones and back.summary == summary
    assert (back.order, back.beam) == (4, 64)
    for k in ("keys", "logp", "bow", "offs", "discounts"):
        assert back.lm[k].dtype == model.lm[k].dtype and back.lm[k].tobytes() == model.lm[k].tobytes()
    for k in ("type_letters", "type_phones", "spell_offs", "spell_types"):
        assert np.array_equal(getattr(back, k), getattr(model, k))


def test_entries_are_skipped_and_counted_by_reason():
    lim = g2p.limits()
    assert (lim["letters"], lim["phones"], lim["word_letters"], lim["word_phones"], lim["order"]) == (64, 128, 32, 48, 4)
    lex = {"ab": ["AA", "B"], "a" * 33: ["AA"], "b": ["B"] * 49, "c": [], "d": ["D", "D", "D"], "ha": ["HH", "AA", "AA"]}
    used, skipped = g2p.select_entries(lex)
    assert [w for w, _ in used] == ["ab", "ha"]
    assert skipped == {"limit": 2, "empty": 1, "no_path": 1}
    with pytest.raises(ValueError):
        g2p.alphabets({chr(0x4e00 + k): ["AA"] for k in range(65)})


def test_text_front_end():
    lexicon = {"hello": ["HH", "AH0", "L", "OW1"], "world": ["W", "ER1", "L", "D"]}
    asked = []

    def pronounce(words):
        asked.append(list(words))
        return [None if any(c.isdigit() for c in w) else [c.upper() for c in w] for w in words]

    fake = types.SimpleNamespace(pronounce=pronounce)
    text, dropped = g2p.text_to_phones("Hello, WORLD ab 42 - cd!?", lexicon, fake)
    assert text == "{HH AH0 L OW1 sp W ER1 L D A B sp C D}"
    assert dropped == ["42"] and asked == [["42", "ab", "cd"]]
    assert g2p.split_text("a.b;c") == [("word", "a"), ("pause", "."), ("word", "b"), ("pause", ";"), ("word", "c")]
    assert g2p.text_to_phones("hello", lexicon, fake) == ("{HH AH0 L OW1}", [])


def test_synthesize_refusal_without_a_model_keeps_its_message():
    import synthesize
    args = synthesize.parse_args(["--restore_step", "1", "--mode", "single", "--text", "free text", "-p", "p", "-m", "m", "-t", "t"])
    with pytest.raises(SystemExit) as e:
        synthesize.single_batch(args, {"preprocessing": {"text": {"text_cleaners": [], "language": "en"}}})
    assert str(e.value) == ("--mode single expects a phoneme string in braces, e.g. --text \"{HH AH0 L OW1 sp W ER1 L D}\" "
                            "(grapheme-to-phoneme conversion needs g2p_en/pypinyin, which this build does not ship)")
    assert args.g2p_model is None


def test_the_reference_alone_stays_within_the_near_tie_allowance(small):
    bars = json.load(open(BARS))
    assert bars["near_tie_share"] <= 0.02 and bars["align_near_ties"] <= 0.02
    assert len(bars["held_out"]) == 40 and all(b >= a for a, b in zip(bars["loglik"], bars["loglik"][1:]))
    m, entries, _, _ = small
    T, words = len(m["tokens"]), g2p_corpus.decode_words(entries[120:], A)
    for N in (1, 2, 4):                                                    # the cases of tests/test_g2p_gpu.py's decoding test
        md = g2p_ref.model_from_arrays(g2p.kneser_ney(m["seqs"], T, N), N)
        for K in (1, 4, 256):
            near = 0
            for w in words:
                got, score, _, gap = g2p_ref.beam_search(w, m["spelling"], md, N, K, T, m["type_phones"])
                near += got is not None and 0.0 < gap < 1e-9 * abs(score)    # an exact tie is decided by the stated rule
            assert near <= 0.02 * len(words), (N, K, near, len(words))
