"""Helix maps for the base-pair score (align_bp_score_slv) from the forms users hold them in.

The score needs, per alignment column, the column it pairs with in the secondary structure.  SINA reads that from the
HELIX data of an ARB database; without ARB the usual form is a dot-bracket line as wide as the alignment, such as the
SS_cons line of a Stockholm file.  Store.set_pairs takes the map this module makes of it.
"""
import numpy as np

_OPEN = {"(": ")", "<": ">", "[": "]", "{": "}"}
_CLOSE = {v: k for k, v in _OPEN.items()}


def pairs_from_brackets(text):
    """The helix map of a dot-bracket line: uint32 [len(text)], pairs[i] = the column paired with column i, 0 = unpaired.

    The brackets (), <>, [] and {} pair up, each kind nested on a stack of its own (so that pseudoknots written with
    a second kind of bracket cross the first); every other character is an unpaired column.  Raises ValueError for a
    bracket that finds no partner, and for a bracket at column 0: a partner of 0 means "unpaired", so a pair with
    column 0 cannot be expressed.
    """
    pairs = np.zeros(len(text), np.uint32)
    stacks = {o: [] for o in _OPEN}
    for i, ch in enumerate(text):
        if ch in _OPEN:
            if i == 0:
                raise ValueError("pairs_from_brackets: a bracket at column 0 cannot be expressed (partner 0 means unpaired)")
            stacks[ch].append(i)
        elif ch in _CLOSE:
            st = stacks[_CLOSE[ch]]
            if not st:
                raise ValueError("pairs_from_brackets: unbalanced %r at column %d" % (ch, i))
            j = st.pop()
            pairs[i] = j
            pairs[j] = i
    for o, st in stacks.items():
        if st:
            raise ValueError("pairs_from_brackets: unbalanced %r at column %d" % (o, st[-1]))
    return pairs
