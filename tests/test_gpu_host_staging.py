"""What the host-pointer forms stage, request by request: the fourteen host forms that share one staging helper (solve, logdet and the
twelve GP families), both dtypes, every output asked for alone, every optional input left out, and every input supplied although the
request does not need it. Each result is compared BITWISE with the device form of the same request, which is handed only the inputs the
request reads -- so a buffer staged under the wrong condition, with the wrong size or in the wrong slot shows. The numbers themselves are
checked by each family's own file; the host form is the same code on every kernel route, so one small size serves here.

Argument lists: tests/test_refusals_cpu.py (FAMILIES). Shapes: n = q = 5, batch 3, 2 right-hand sides, 2 targets, 3 query points,
2 samples / points, 2 derivative matrices, 2 basis functions."""
import ctypes
import functools

import numpy as np
import pytest

import test_refusals_cpu as R
from conftest import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
api = pkg("api")
lib = pkg("_lib")
N, BATCH, NRHS, D, Q, S, P, K = 5, 3, 2, 2, 3, 2, 2, 2
DTYPES = ("float64", "float32")
SCALARS = dict(algo=api.ALGO_GAUSS_JORDAN, n=N, q=N, nrhs=NRHS, D=D, Q=Q, S=S, P=P, K=K, sA=N * N, sB=N * NRHS, sX=N * NRHS, strideC=N * N)
REQUIRED = dict(solve=("X",), logdet=("logabsdet",), sample=("Y",))  # the outputs a family always computes
# the inputs a caller may leave out altogether (sample without Ds: the zero-mean posterior, which has no mean output; sample keeps its Es:
# without a prior covariance the predictive covariance is not positive definite and info says so)
OPTIONAL_INPUTS = dict(logml="C", loo="C", logml_grad="C", loo_grad="C", predict="CE", predict_cov="CE", colour="M", whiten="M",
                       multi_target="C", multi_target_grad="C", trend="C", sample="CD")


def needed(fam, want):
    """the inputs that the request `want` reads, by the contract of include/matinv.h: what the host form has to stage, and no more"""
    w = set(want)
    skip = set()
    if fam in ("logml_grad", "loo_grad", "multi_target_grad") and "grad" not in w:
        skip |= {"DM"}
    if fam in ("predict", "predict_cov"):
        skip |= ({"D"} if "mean" not in w else set()) | ({"E"} if not w & {"var", "cov"} else set())
    if fam == "colour" and "Y" not in w:
        skip |= {"M", "Z"}
    if fam == "whiten" and not w & {"W", "maha", "logpdf"}:
        skip |= {"M", "X"}
    if fam == "multi_target":
        skip |= ({"Y"} if not w & {"alpha", "quad", "logml", "mean"} else set()) | ({"A"} if "mean" not in w else set())
    if fam == "trend":
        skip |= ({"Y"} if not w & {"beta", "alpha", "quad", "logml", "mean"} else set()) | ({"A", "G"} if not w & {"mean", "var"} else set())
        skip |= {"E"} if "var" not in w else set()
    f = R.FAMILIES[fam]
    return [p for p in f.pointers if p not in f.outputs and p != "sign" and p not in skip]


@functools.lru_cache(maxsize=None)
def case(fam, dtname):
    """(inputs, output sizes) of one family: seeded numpy, SPD matrices well away from singular, so that info is all zero"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng(sorted(R.FAMILIES).index(fam))

    def rand(*shape):
        return rng.standard_normal(shape).reshape(-1).astype(dt)

    def spd(m, count, shift):
        r = rng.random((count, m, m))
        return (r @ r.transpose(0, 2, 1) + shift * np.eye(m)).reshape(-1).astype(dt)

    def sym(m, count):
        r = rng.standard_normal((count, m, m))
        return (r + r.transpose(0, 2, 1)).reshape(-1).astype(dt)

    vec, mat = BATCH * N, BATCH * N * N
    gp = dict(B=spd(N, BATCH, N), C=rng.uniform(0.1, 1.0, vec).astype(dt), D=rand(vec))
    queries = dict(A=rand(BATCH * Q * N))
    if fam == "solve":
        return dict(A=spd(N, BATCH, N), B=rand(BATCH * N * NRHS)), dict(X=BATCH * N * NRHS)
    if fam == "logdet":
        return dict(A=spd(N, BATCH, N)), dict(logabsdet=BATCH, sign=BATCH)
    if fam == "logml":
        return gp, dict(logml=BATCH)
    if fam == "loo":
        return gp, dict(mean=vec, var=vec, logpl=BATCH)
    if fam == "logml_grad":
        return dict(gp, DM=sym(N, BATCH * P)), dict(grad=BATCH * P, gradc=vec, alpha=vec)
    if fam == "loo_grad":
        return dict(gp, DM=sym(N, BATCH * P)), dict(grad=BATCH * P, gradc=vec, logpl=BATCH)
    if fam == "predict":
        return dict(gp, **queries, E=rng.uniform(1.0, 2.0, BATCH * Q).astype(dt)), dict(mean=BATCH * Q, var=BATCH * Q)
    if fam == "predict_cov":
        return dict(gp, **queries, E=spd(Q, BATCH, 10)), dict(mean=BATCH * Q, cov=BATCH * Q * Q)
    if fam == "colour":
        return dict(C=spd(N, BATCH, N), M=rand(vec), Z=rand(BATCH * S * N)), dict(Y=BATCH * S * N, L=mat)
    if fam == "whiten":
        return (dict(C=spd(N, BATCH, N), M=rand(vec), X=rand(BATCH * S * N)),
                dict(W=BATCH * S * N, maha=BATCH * S, logdet=BATCH, logpdf=BATCH * S))
    if fam == "multi_target":
        return (dict(B=gp["B"], C=gp["C"], Y=rand(BATCH * D * N), **queries),
                dict(alpha=BATCH * D * N, quad=BATCH * D, logdet=BATCH, logml=BATCH * D, mean=BATCH * D * Q))
    if fam == "multi_target_grad":
        return (dict(B=gp["B"], C=gp["C"], Y=rand(BATCH * D * N), DM=sym(N, BATCH * P)),
                dict(grad=BATCH * P, gradc=vec, logml=BATCH * D, alpha=BATCH * D * N))
    if fam == "trend":
        return (dict(B=gp["B"], C=gp["C"], H=rand(BATCH * K * N), Y=rand(BATCH * D * N), **queries, G=rand(BATCH * Q * K),
                     E=rng.uniform(1.0, 2.0, BATCH * Q).astype(dt)),
                dict(beta=BATCH * D * K, covbeta=BATCH * K * K, alpha=BATCH * D * N, quad=BATCH * D, logml=BATCH * D, mean=BATCH * D * Q,
                     var=BATCH * Q))
    if fam == "sample":
        return dict(gp, **queries, E=spd(Q, BATCH, 10), Z=rand(BATCH * S * Q)), dict(Y=BATCH * S * Q, mean=BATCH * Q, cov=BATCH * Q * Q)
    raise KeyError(fam)


def requests(fam):
    """(want, inputs left out): everything; every other output alone; everything that is left without each optional input"""
    f = R.FAMILIES[fam]
    outputs = tuple(p for p in f.pointers if p in f.outputs or p == "sign")
    base = REQUIRED.get(fam, ())
    out = [(outputs, ())]
    for want in ([base] if base else []) + [base + (o,) for o in outputs if o not in base]:
        if (want, ()) not in out:
            out.append((want, ()))
    for name in OPTIONAL_INPUTS.get(fam, ""):
        out.append((tuple(o for o in outputs if not (fam == "sample" and name == "D" and o == "mean")), (name,)))
    if len(OPTIONAL_INPUTS.get(fam, "")) > 1:
        out.append((tuple(o for o in outputs if not (fam == "sample" and o == "mean")), tuple(OPTIONAL_INPUTS[fam])))
    return out


def call(fam, dtname, form, want, given, with_info=True):
    """one raw call of the C ABI: (outputs by name as numpy arrays, info or None). `given`: the inputs handed over."""
    f = R.FAMILIES[fam]
    inputs, sizes = case(fam, dtname)
    scalars = {k: SCALARS.get(k, lib.F64 if dtname == "float64" else lib.F32) for k in f.scalars}
    if form == "dev":
        hold = {k: torch.tensor(inputs[k]).cuda() for k in given}
        outs = {k: torch.full((sizes[k],), float("nan"), dtype=getattr(torch, dtname), device="cuda") for k in want}
        info = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda") if with_info else None
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    else:
        hold = {k: inputs[k].copy() for k in given}
        outs = {k: np.full(sizes[k], np.nan, dtype=dtname) for k in want}
        info = np.full(BATCH, -7, dtype=np.int32) if with_info else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    pointers = {k: ptr(outs.get(k, hold.get(k))) for k in f.pointers}
    lib.check(f.function(lib.lib(), form)(*f.args(form, scalars, pointers, BATCH, ptr(info))))
    if form == "dev":
        torch.cuda.synchronize()
        outs = {k: v.cpu().numpy() for k, v in outs.items()}
        hold = {k: v.cpu().numpy() for k, v in hold.items()}
        info = None if info is None else info.cpu().numpy()
    for k, v in hold.items():
        assert v.tobytes() == inputs[k].tobytes(), f"{fam} {form}: input {k} was modified"
    return outs, info


@functools.lru_cache(maxsize=None)
def device_form(fam, dtname, want, left_out):
    """the device form of a request, handed the inputs that the request reads and nothing else; shared by the tests, never modified"""
    outs, info = call(fam, dtname, "dev", want, [k for k in needed(fam, want) if k not in left_out])
    assert not info.any(), (fam, dtname, want, info)
    for k, v in outs.items():
        assert not np.isnan(v).any(), f"{fam} dev: {k} was not written everywhere"
    return outs


def same(fam, dtname, want, got, what):
    ref = device_form(fam, dtname, want, ())
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].tobytes() == ref[k].tobytes(), f"{fam} {dtname} {what}: {k} differs from the device form (want={want})"


@pytest.mark.parametrize("dtname", DTYPES)
@pytest.mark.parametrize("fam", sorted(R.FAMILIES))
def test_every_request_of_the_host_form_equals_the_device_form(fam, dtname):
    """the host form is handed EVERY input it is not told to do without, whatever the request: what the request does not read must be
    neither needed nor harmful"""
    inputs, _ = case(fam, dtname)
    assert len(requests(fam)) >= (1 if fam in ("solve", "logml") else 2)
    for want, left_out in requests(fam):
        got, info = call(fam, dtname, "host", want, [k for k in inputs if k not in left_out])
        assert not info.any(), (fam, want, left_out, info)
        ref = device_form(fam, dtname, want, left_out)
        for k in want:
            assert got[k].tobytes() == ref[k].tobytes(), f"{fam} {dtname}: {k} differs from the device form (want={want}, without {left_out})"


@pytest.mark.parametrize("dtname", DTYPES)
@pytest.mark.parametrize("fam", sorted(R.FAMILIES))
def test_info_may_be_null(fam, dtname):
    inputs, sizes = case(fam, dtname)
    want = tuple(sizes)
    got, info = call(fam, dtname, "host", want, list(inputs), with_info=False)
    assert info is None
    same(fam, dtname, want, got, "info = NULL")


def api_host(fam, i, want):
    """the family's api.*_batched_host call with every input; returns (its outputs by name, info)"""
    g = i.get
    if fam == "solve":
        x, info = api.solve_batched_host(i["A"], i["B"], N, NRHS)
        return dict(X=x), info
    if fam == "logdet":
        sign, logabsdet, info = api.logdet_batched_host(i["A"], N)
        return dict(logabsdet=logabsdet, sign=sign), info
    names = R.FAMILIES[fam].outputs
    if fam == "logml":
        res = api.logml_batched_host(N, i["B"], g("C"), i["D"])
    elif fam == "loo":
        res = api.loo_batched_host(N, i["B"], g("C"), i["D"])
    elif fam == "logml_grad":
        res = api.logml_grad_batched_host(N, i["B"], g("C"), i["D"], i["DM"], want=want)
    elif fam == "loo_grad":
        res = api.loo_grad_batched_host(N, i["B"], g("C"), i["D"], i["DM"], want=want)
    elif fam == "predict":
        res = api.predict_batched_host(N, i["B"], g("C"), i["D"], i["A"], g("E"), want=want)
    elif fam == "predict_cov":
        res = api.predict_cov_batched_host(N, i["B"], g("C"), i["D"], i["A"], g("E"), want=want)
    elif fam == "colour":
        res = api.colour_batched_host(N, i["C"], g("M"), i["Z"], want=want)
    elif fam == "whiten":
        res = api.whiten_batched_host(N, i["C"], g("M"), i["X"], want=want)
    elif fam == "multi_target":
        res = api.multi_target_batched_host(N, i["B"], g("C"), i["Y"], i["A"], want=want)
    elif fam == "multi_target_grad":
        res = api.multi_target_grad_batched_host(N, i["B"], g("C"), i["Y"], i["DM"], want=want)
    elif fam == "trend":
        res = api.trend_batched_host(N, i["B"], g("C"), i["H"], i["Y"], i["A"], i["G"], i["E"], want=want)
    else:
        res = api.sample_batched_host(N, i["B"], g("C"), g("D"), i["A"], g("E"), i["Z"], want=want)
    return dict(zip(names, res[:-1])), res[-1]


@pytest.mark.parametrize("dtname", DTYPES)
@pytest.mark.parametrize("fam", sorted(R.FAMILIES))
def test_api_host_forms_return_what_was_asked_for_and_nothing_else(fam, dtname):
    """through the Python wrappers, with every input supplied: predict with Es and want=("mean",), colour with Ms and want=("L",),
    whiten with Ms, Xs and want=("logdet",), multi_target with Ys, As and want=("logdet",), trend with all inputs and
    want=("covbeta",), sample with Ds = None, ... -- an output not in want comes back None, the others equal the device form"""
    inputs, sizes = case(fam, dtname)
    has_want = fam not in ("solve", "logdet", "logml", "loo")
    for want, left_out in requests(fam) if has_want else [(tuple(sizes), ())]:
        got, info = api_host(fam, {k: v for k, v in inputs.items() if k not in left_out}, want)
        assert info.dtype == np.int32 and info.shape == (BATCH,) and not info.any()
        ref = device_form(fam, dtname, want, left_out)
        for k in sizes:
            if k not in want:
                assert got[k] is None, f"{fam}: {k} was not asked for (want={want})"
            else:
                assert got[k].tobytes() == ref[k].tobytes(), f"{fam} {dtname}: api {k} differs from the device form (want={want}, without {left_out})"
