"""scripts/entry_trace.py writes a scenario's entry calls folded (repeated blocks once): folding must lose nothing, or two trees with
different call sequences could compare equal."""
import importlib.util
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("entry_trace", os.path.join(ROOT, "scripts", "entry_trace.py"))
entry_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(entry_trace)


def unfold(text):
    toks = re.findall(r"\[|\]\*\d+|[^\s\[\]]+", text)

    def parse(i):
        out = []
        while i < len(toks) and not toks[i].startswith("]*"):
            if toks[i] == "[":
                inner, i = parse(i + 1)
                out += inner * int(toks[i][2:])
            else:
                m = re.fullmatch(r"(.+)\*(\d+)", toks[i])
                out += [m.group(1)] * int(m.group(2)) if m else [toks[i]]
            i += 1
        return out, i
    return parse(0)[0]


def test_fold_writes_repeats_once_and_unfolds_to_the_same_list():
    fold = entry_trace.fold
    assert fold([]) == [] and fold(["a"]) == ["a"] and fold(["a", "b", "c"]) == ["a", "b", "c"]
    assert fold(["a", "a", "a"]) == ["a*3"] and fold(["c", "d", "d", "a"]) == ["c", "d*2", "a"]
    assert fold(["+x", "y"] * 3 + ["z"]) == ["[+x y]*3", "z"]
    assert fold((["a", "b", "b"] * 2 + ["c"]) * 2) == ["[[a b*2]*2 c]*2"]
    rng = random.Random(0)
    for _ in range(1000):
        base = [rng.choice(["a", "+b", "rfx_c_f32", "d"]) for _ in range(rng.randint(0, 12))]
        names = []
        for _ in range(rng.randint(1, 4)):
            names += base[:rng.randint(0, len(base))] * rng.randint(1, 4)
        assert unfold(" ".join(fold(names))) == names, names
