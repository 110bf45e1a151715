"""Every refusal of the solve, logdet and GP entry points of the C ABI, device and host form alike, byte for byte: the return code and
the full text of matinv_last_error() of each call below are compared with tests/golden/refusals.json. The per-family CPU tests look for
substrings; this one fails when a shared helper changes one family's wording or the order of its checks.

The table is recorded from a library built at the commit BEFORE a change of the argument checks, never from the code under test:
    MATINV_LIB=/path/to/that/libmatinv_hip.so python tests/test_refusals_cpu.py --record
Only calls that are refused before the device is looked at, and empty batches, belong here: the pointers are never read. No GPU needed."""
import ctypes
import json
import os
import sys

import pytest

from conftest import GOLDEN, pkg

TABLE = os.path.join(GOLDEN, "refusals.json")
BIG = 0x80000000  # one more than the grid limit


class Family:
    """The argument list of matinv_<name>_batched and matinv_<name>_batched_host. `order` names the arguments between the first one and
    `batch`: a scalar (a key of `scalars`, which holds the defaults), a pointer (anything else) or ("dev", scalar) for an argument that
    only the device form has. `outputs`: the pointers whose absence means "not asked for". `size`: what the family calls its order."""

    def __init__(self, name, order, scalars, outputs, size="n"):
        self.name, self.order, self.scalars, self.outputs, self.size = name, order, scalars, outputs, size
        self.pointers = [t for t in order if not isinstance(t, tuple) and t not in scalars]

    def args(self, form, scalars, pointers, batch, info, stream=None):
        """the ctypes argument list of one call; pointers: name -> c_void_p or None"""
        out = []
        for tok in self.order:
            if isinstance(tok, tuple):
                if form == "dev":
                    out.append(scalars[tok[1]])
            elif tok in self.scalars:
                out.append(scalars[tok])
            else:
                out.append(pointers[tok])
        return out + [batch, info] + ([stream] if form == "dev" else [])

    def function(self, L, form):
        return getattr(L, f"matinv_{self.name}_batched" + ("_host" if form == "host" else ""))


FAMILIES = {f.name: f for f in (
    Family("solve", ["algo", "dtype", "n", "nrhs", "A", ("dev", "sA"), "B", ("dev", "sB"), "X", ("dev", "sX")],
           dict(algo=0, dtype=0, n=4, nrhs=2, sA=16, sB=8, sX=8), ("X",)),
    Family("logdet", ["algo", "dtype", "n", "A", ("dev", "sA"), "logabsdet", "sign"], dict(algo=0, dtype=0, n=4, sA=16), ("logabsdet",)),
    Family("logml", ["dtype", "n", "B", "C", "D", "logml"], dict(dtype=0, n=4), ("logml",)),
    Family("loo", ["dtype", "n", "B", "C", "D", "mean", "var", "logpl"], dict(dtype=0, n=4), ("mean", "var", "logpl")),
    Family("logml_grad", ["dtype", "n", "P", "B", "C", "D", "DM", "grad", "gradc", "alpha"], dict(dtype=0, n=4, P=2),
           ("grad", "gradc", "alpha")),
    Family("loo_grad", ["dtype", "n", "P", "B", "C", "D", "DM", "grad", "gradc", "logpl"], dict(dtype=0, n=4, P=2),
           ("grad", "gradc", "logpl")),
    Family("predict", ["dtype", "n", "Q", "B", "C", "D", "A", "E", "mean", "var"], dict(dtype=0, n=4, Q=2), ("mean", "var")),
    Family("predict_cov", ["dtype", "n", "Q", "B", "C", "D", "A", "E", "mean", "cov"], dict(dtype=0, n=4, Q=2), ("mean", "cov")),
    Family("colour", ["dtype", "q", "S", "C", "strideC", "M", "Z", "Y", "L"], dict(dtype=0, q=4, S=2, strideC=16), ("Y", "L"), size="q"),
    Family("whiten", ["dtype", "q", "S", "C", "strideC", "M", "X", "W", "maha", "logdet", "logpdf"], dict(dtype=0, q=4, S=2, strideC=16),
           ("W", "maha", "logdet", "logpdf"), size="q"),
    Family("multi_target", ["dtype", "n", "D", "Q", "B", "C", "Y", "A", "alpha", "quad", "logdet", "logml", "mean"],
           dict(dtype=0, n=4, D=2, Q=2), ("alpha", "quad", "logdet", "logml", "mean")),
    Family("multi_target_grad", ["dtype", "n", "D", "P", "B", "C", "Y", "DM", "grad", "gradc", "logml", "alpha"],
           dict(dtype=0, n=4, D=2, P=2), ("grad", "gradc", "logml", "alpha")),
    Family("trend", ["dtype", "n", "K", "D", "Q", "B", "C", "H", "Y", "A", "G", "E", "beta", "covbeta", "alpha", "quad", "logml", "mean", "var"],
           dict(dtype=0, n=4, K=2, D=2, Q=2), ("beta", "covbeta", "alpha", "quad", "logml", "mean", "var")),
    Family("sample", ["dtype", "n", "Q", "S", "B", "C", "D", "A", "E", "Z", "Y", "mean", "cov"], dict(dtype=0, n=4, Q=2, S=2),
           ("Y", "mean", "cov")),
)}


def only(fam, *kept):
    """the overrides that ask for the outputs `kept` alone"""
    return {k: None for k in FAMILIES[fam].outputs if k not in kept}


def shared(fam):
    """what every family refuses alike: order, dtype, the empty batch, the first pointer, no output, the grid limit, the order limit, and
    the mixed cases that pin the order of these checks"""
    f = FAMILIES[fam]
    s, first = f.size, f.pointers[0]
    nothing, no_output = dict.fromkeys(f.pointers), dict.fromkeys(f.outputs)
    # an order of 1025 with strides that pass: the device forms of solve and logdet, colour and whiten check their strides first
    wide = {s: 1025, **{k: 1025 * 1025 for k in ("sA", "sB", "sX", "strideC") if k in f.scalars}}
    return [{s: 0}, {s: -3}, {"dtype": 2}, {"dtype": -1}, {s: 0, "dtype": 2},
            {"batch": 0, **nothing}, {"batch": 0, "dtype": 5, **nothing}, {"batch": 0, s: 0, **nothing}, {"batch": 0, s: 0, "dtype": 5},
            {first: None}, no_output, {first: None, **no_output},
            {"batch": BIG}, {"batch": BIG, **no_output}, {"batch": BIG, first: None},
            {s: 1025}, wide, {**wide, first: None}, {**wide, **no_output}, {**wide, "batch": BIG}]


def own(fam):
    """each family's own lines: counts, pointers, "X requested without Y", limits, and the mixed cases that pin their order"""
    none = dict.fromkeys(FAMILIES[fam].outputs)
    if fam == "solve":
        return [{"nrhs": 0}, {"nrhs": 0, "algo": 7}, {"n": 0, "nrhs": 0}, {"algo": 7}, {"algo": 7, "dtype": 2}, {"B": None}, {"A": None, "B": None},
                {"sA": 15}, {"sB": 7}, {"sX": 7}, {"sA": 15, "A": None}, {"sA": 15, "batch": BIG}, {"sA": 15, "batch": 1, "n": 1025},
                {"batch": 0, "algo": 7}, {"batch": 0, "nrhs": 0}]
    if fam == "logdet":
        return [{"algo": 7}, {"algo": 7, "dtype": 2}, {"n": 0, "algo": 7}, {"sA": 15}, {"sA": 15, "A": None}, {"sA": 15, "batch": BIG},
                {"sA": 15, "batch": 1, "n": 1025}, {"batch": 0, "algo": 7}]
    if fam == "logml":
        return [{"D": None}, {"D": None, "n": 1025}]
    if fam == "loo":
        return [{"D": None}, {"D": None, **none}, {"D": None, "n": 1025}]
    if fam in ("logml_grad", "loo_grad"):
        return [{"P": -1}, {"P": -1, "B": None}, {"P": -1, **none}, {"P": -1, **only(fam, "gradc")}, {"D": None}, {"D": None, **none},
                {"P": 0}, {"P": 0, "DM": None}, {"P": 0, **only(fam, "grad")}, {"DM": None}, {"DM": None, **only(fam, "grad")},
                {"DM": None, "n": 1025}, {"DM": None, "batch": BIG}, {"P": 0, "B": None}]
    if fam in ("predict", "predict_cov"):
        second = FAMILIES[fam].outputs[1]
        more = [{"Q": 1025}, {"Q": 1025, "n": 1025}, {"Q": 1025, "batch": BIG}, {"Q": 1025, **only(fam, second)},
                {"Q": 1025, "D": None}] if fam == "predict_cov" else []
        return [{"Q": 0}, {"Q": -1}, {"Q": 0, "A": None}, {"Q": 0, **none}, {"A": None}, {"A": None, **none}, {"D": None},
                {"D": None, **only(fam, "mean")}, {"D": None, **none}, {"D": None, "n": 1025}, {"D": None, "batch": BIG}] + more
    if fam == "colour":
        wide = {"q": 1025, "strideC": 1025 * 1025}
        return [{"Z": None}, {"Z": None, **only(fam, "Y")}, {"Z": None, **none}, {"S": 0}, {"S": -1, **only(fam, "Y")}, {"S": 0, "Z": None},
                {"strideC": 15}, {"strideC": 0}, {"strideC": 15, "S": 0}, {"strideC": 15, "batch": BIG}, {"strideC": 15, **only(fam, "L")},
                {"S": 1025}, {"S": 1025, **only(fam, "Y")}, {"S": 1025, **wide}, {"S": 1025, "batch": BIG}, {"S": 1025, "strideC": 15}]
    if fam == "whiten":
        wide = {"q": 1025, "strideC": 1025 * 1025}
        each = [c for one in ("W", "maha", "logpdf") for c in ({"X": None, **only(fam, one)}, {"S": 0, **only(fam, one)},
                                                                {"S": 1025, **only(fam, one)})]
        return each + [{"X": None}, {"X": None, **none}, {"S": 0}, {"S": 0, "X": None}, {"strideC": 15}, {"strideC": 15, "S": 0},
                       {"strideC": 15, "batch": BIG}, {"strideC": 15, **only(fam, "logdet")}, {"S": 1025}, {"S": 1025, **wide},
                       {"S": 1025, "batch": BIG}, {"S": 1025, "strideC": 15}, {**wide, **only(fam, "logdet")}]
    if fam == "multi_target":
        each = [c for one in ("alpha", "quad", "logml", "mean") for c in ({"Y": None, **only(fam, one)}, {"D": 0, **only(fam, one)},
                                                                          {"D": 1025, **only(fam, one)})]
        return each + [{"A": None, **only(fam, "mean")}, {"Q": 0, **only(fam, "mean")}, {"Q": 1025, **only(fam, "mean")},
                       {"Y": None}, {"A": None}, {"D": 0}, {"Q": 0}, {"D": 0, "Q": 0}, {"D": 0, "B": None}, {"Q": 0, "A": None},
                       {"Y": None, "A": None}, {"Y": None, "B": None}, {"D": 0, **none}, {"D": 1025}, {"Q": 1025}, {"D": 1025, "Q": 1025},
                       {"D": 1025, "n": 1025}, {"D": 1025, "batch": BIG}, {"D": 1025, "Y": None}, {"n": 1025, **only(fam, "logdet")}]
    if fam == "multi_target_grad":
        return [{"D": 0}, {"D": -1, **only(fam, "alpha")}, {"P": -1}, {"P": -1, **only(fam, "logml")}, {"P": 0}, {"P": 0, **only(fam, "grad")},
                {"D": 0, "P": -1}, {"D": 0, "B": None}, {"P": 0, "B": None}, {"Y": None}, {"Y": None, **none}, {"Y": None, "DM": None},
                {"DM": None}, {"DM": None, **only(fam, "grad")}, {"DM": None, "n": 1025}, {"D": 1025}, {"P": 1025}, {"D": 1025, "P": 1025},
                {"D": 1025, "n": 1025}, {"P": 1025, "batch": BIG}, {"D": 1025, **only(fam, "gradc")}, {"P": 1025, "DM": None}]
    if fam == "trend":
        out = [{"n": 32, "K": K} for K in (0, -1, 17)] + [{"K": 5}, {"K": 5, "dtype": 2}, {"K": 5, "n": 0}, {"K": 0, "B": None}]
        for one in ("beta", "alpha", "quad", "logml", "mean"):
            out += [{"Y": None, **only(fam, one)}, {"D": 0, **only(fam, one)}, {"D": 1025, **only(fam, one)}]
        for one in ("mean", "var"):
            out += [{"A": None, **only(fam, one)}, {"G": None, **only(fam, one)}, {"Q": 0, **only(fam, one)}, {"Q": 1025, **only(fam, one)}]
        return out + [{"H": None}, {"H": None, **none}, {"E": None}, {"E": None, **only(fam, "var")}, {"Y": None}, {"A": None}, {"G": None},
                      {"A": None, "G": None}, {"D": 0}, {"Q": 0}, {"Q": 0, "A": None}, {"D": 0, "Q": 0}, {"D": 0, "H": None},
                      {"Y": None, "A": None}, {"G": None, "E": None}, {"batch": 0, "K": 17, "n": 32, **dict.fromkeys(FAMILIES[fam].pointers)},
                      {"batch": 0, "K": 5}, {"n": 1025, "D": 0, "Q": 0, "Y": None, "A": None, "G": None, "E": None, **only(fam, "covbeta")},
                      {"D": 1025}, {"Q": 1025}, {"D": 1025, "Q": 1025}, {"D": 1025, "n": 1025}, {"Q": 1025, "batch": BIG}, {"E": None, "n": 1025}]
    if fam == "sample":
        return [{"Q": 0}, {"S": 0}, {"Q": 0, "S": 0}, {"Q": 0, "A": None}, {"S": 0, "Z": None}, {"A": None}, {"Z": None}, {"A": None, "Y": None},
                {"Y": None}, {"Y": None, "D": None}, {"D": None}, {"D": None, **only(fam, "Y", "mean")}, {"D": None, "n": 1025},
                {"D": None, "batch": BIG}, {"Q": 1025}, {"S": 1025}, {"Q": 1025, "S": 1025}, {"Q": 1025, "n": 1025}, {"S": 1025, "batch": BIG},
                {"Q": 1025, "D": None}]
    raise KeyError(fam)


def call_id(fam, form, over):
    return f"{fam}.{form}(" + ", ".join(f"{k}={'NULL' if v is None else v}" for k, v in sorted(over.items())) + ")"


def calls():
    """id -> (family, form, overrides); an override of an argument the host form does not have is dropped there"""
    out = {}
    for fam, f in FAMILIES.items():
        dev_only = {t[1] for t in f.order if isinstance(t, tuple)}
        for over in shared(fam) + own(fam):
            for form in ("dev", "host"):
                o = {k: v for k, v in over.items() if form == "dev" or k not in dev_only}
                if o:  # nothing left: the call was about a stride, which the host form derives
                    out[call_id(fam, form, o)] = (fam, form, o)
    return out


def run(L, fam, form, over):
    """(rc, message): the message is None for a call that succeeded -- matinv_last_error() then still holds an older one"""
    f = FAMILIES[fam]
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    scalars = {k: over.get(k, v) for k, v in f.scalars.items()}
    pointers = {k: over.get(k, p) for k in f.pointers}
    batch = over.get("batch", 2)
    rc = f.function(L, form)(*f.args(form, scalars, pointers, batch, None))
    lib = pkg("_lib")
    # nothing here may reach the device: a call is refused for its arguments, or its batch is empty
    assert rc in (lib.ERR_ARG, lib.ERR_UNSUPPORTED) or (rc == lib.OK and batch == 0), (call_id(fam, form, over), rc, L.matinv_last_error())
    return rc, (None if rc == lib.OK else L.matinv_last_error().decode())


def test_the_recorded_table_holds_exactly_the_calls_of_this_file():
    table = json.load(open(TABLE))["calls"]
    assert sorted(table) == sorted(calls())
    # every family in both forms, and nothing that would have needed a device
    assert {i.split("(")[0] for i in table} == {f"{fam}.{form}" for fam in FAMILIES for form in ("dev", "host")}
    assert all(rc in (-1, -2) and msg or (rc == 0 and msg is None and "batch=0" in i) for i, (rc, msg) in table.items())


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_every_refusal_is_the_recorded_one_byte_for_byte(fam):
    L = pkg("_lib").lib()
    table = json.load(open(TABLE))["calls"]
    mine = {i: c for i, c in calls().items() if c[0] == fam}
    assert len(mine) >= 2 * len(shared(fam))
    wrong = {}
    for i, (_, form, over) in mine.items():
        got = list(run(L, fam, form, over))
        if got != table[i]:
            wrong[i] = dict(got=got, recorded=table[i])
    assert not wrong, json.dumps(wrong, indent=1)


def test_device_and_host_form_refuse_alike():
    """one *_check_args serves both forms of a family: where both take the same arguments (solve and logdet derive the strides of their
    host form), the recorded answers are the same"""
    table = json.load(open(TABLE))["calls"]
    for i, (fam, form, over) in calls().items():
        if form == "host" and not any(isinstance(t, tuple) for t in FAMILIES[fam].order):
            assert table[i] == table[call_id(fam, "dev", over)], i


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"] or not os.environ.get("MATINV_LIB"):
        sys.exit("usage: MATINV_LIB=<library built at the parent commit> python tests/test_refusals_cpu.py --record")
    L = pkg("_lib").lib()
    recorded = {i: run(L, *c) for i, c in calls().items()}
    with open(TABLE, "w") as fh:
        json.dump(dict(note="recorded by tests/test_refusals_cpu.py --record from a library built before the change under test",
                       calls=recorded), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(recorded)} calls recorded in {TABLE}")
