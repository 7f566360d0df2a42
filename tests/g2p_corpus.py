"""A seeded synthetic lexicon for the grapheme-to-phoneme tests: about 400 words of 1 to 9 letters over the 6 letters `abcdeh` and
the 8 phones AA B CH D EH HH K S.  Pronunciations come from a rule table, left to right:
    ch -> CH                       a digraph: two letters, one phone
    h  -> HH AA                    one letter, two phones (an h that is not part of ch)
    e  -> nothing at the end of a word of two or more letters when the letter before it is b, c or d; else EH
    c  -> S before e, else K       the phone depends on the next letter
    a -> AA, b -> B, d -> D
and about 5 % of the words are exceptions: one phone of the regular pronunciation is replaced by another."""
import numpy as np

LETTERS = "abcdeh"
PHONES = ["AA", "B", "CH", "D", "EH", "HH", "K", "S"]


def regular(word):
    out, i = [], 0
    while i < len(word):
        ch, nxt = word[i], word[i + 1] if i + 1 < len(word) else ""
        if ch == "c" and nxt == "h":
            out.append("CH")
            i += 1
        elif ch == "h":
            out += ["HH", "AA"]
        elif ch == "e":
            if not (i == len(word) - 1 and i >= 1 and word[i - 1] in "bcd"):
                out.append("EH")
        elif ch == "c":
            out.append("S" if nxt == "e" else "K")
        else:
            out.append({"a": "AA", "b": "B", "d": "D"}[ch])
        i += 1
    return out


def lexicon(seed=0, n=400):
    """-> {word: phones}, insertion order fixed by the seed; words with an empty pronunciation do not occur"""
    rng = np.random.RandomState(seed)
    lex = {}
    while len(lex) < n:
        word = "".join(LETTERS[k] for k in rng.randint(0, len(LETTERS), rng.randint(1, 10)))
        pron = regular(word)
        if word in lex or not pron:
            continue
        if rng.rand() < 0.05:
            k = rng.randint(0, len(pron))
            pron[k] = PHONES[(PHONES.index(pron[k]) + 1 + rng.randint(0, len(PHONES) - 1)) % len(PHONES)]
        lex[word] = pron
    return lex


def ids(lex):
    """-> [(letter ids, phone ids)] over the sorted alphabets of the lexicon"""
    letters = sorted({c for w in lex for c in w})
    phones = sorted({p for ps in lex.values() for p in ps})
    return [([letters.index(c) for c in w], [phones.index(p) for p in ps]) for w, ps in lex.items()], letters, phones


def decode_words(held, A=len(LETTERS)):
    """The words of the decoding tests, as letter ids: held-out words, a 1-letter word, a word at the length maximum (32), a word with
    an unknown letter (-1), two words whose only spelling needs a letter nothing spells (id A), every 1-letter word, a third of the
    2-letter words and a dozen 3-letter words."""
    rng = np.random.RandomState(9)
    words = [list(e[0]) for e in held] + [[2], rng.randint(0, A, 32).tolist(), [0, -1, 3], [1, A], [A]]
    words += [[a] for a in range(A)] + [[a, b] for a in range(A) for b in range(A)][::3] + [rng.randint(0, A, 3).tolist() for _ in range(12)]
    return words
