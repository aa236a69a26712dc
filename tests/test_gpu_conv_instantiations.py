"""Every conv kernel instantiation the library holds (tests/golden/conv_instantiations.json; tests/test_conv_instantiation_ledger.py
holds that list to the built library) runs at least once in a small deterministic case and its result matches float64.

Each template argument switches real code -- the padded edge path, the transposed or row-major epilogue, the pooled epilogue, the
second column half, the fused first-layer staging -- and kernel selection (conv_select.h) sends a user's Keras file to any of
them.  Per instantiation: (a) the case the ledger names launched it (ctx.prof_instances(), launches >= 1); (b) the case's output is
within the project's bound of a float64 evaluation of the same layers, the finite mask equal (tests/instantiation_cases.py has the
cases, the bounds and where each bound comes from); where the case sets iss_set_diag bits to reach the instantiation, the same call
without them gives the same result to 5e-5.  A case runs once however many instantiations point at it."""
import json

import pytest

import instantiation_cases as IC
from test_conv_instantiation_ledger import LEDGER, LI

pytestmark = pytest.mark.gpu

with open(LEDGER) as _f:
    _LEDGER = json.load(_f)
_REACHABLE = sorted(k for k, v in _LEDGER.items() if isinstance(v, str))


@pytest.mark.parametrize('inst', _REACHABLE)
def test_instantiation_runs_and_matches_float64(ctx, inst):
    case = _LEDGER[inst]
    r = IC.run_case(ctx, case)
    ran = {LI.canonical_of_profiler_name(k): n for k, n in r['insts'].items()}
    print(f"{inst} | {case} | {r['mode']} | {r['metric']} {r['err']:.2e} | bound {r['bound']:.0e} | parity {r['parity']} | dead windows {r['dead']}")
    assert ran.get(inst, 0) >= 1, (inst, case, sorted(r['insts']))
    assert r['ok'], (inst, case, 'finite mask / x-vector rule')
    assert r['err'] < r['bound'], (inst, case, r['err'], r['bound'])
    if r['parity'] is not None:
        assert r['parity'] < IC.PARITY_BOUND, (inst, case, r['parity'])

