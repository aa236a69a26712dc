"""The ledger of compiled conv kernel instantiations (tests/golden/conv_instantiations.json) against what the built library holds
(tools/list_conv_instantiations.py reads its symbol table): equal in both directions, so a template instantiation added to a
launcher without a float64 case of its own (tests/instantiation_cases.py, run by tests/test_gpu_conv_instantiations.py) fails here,
on a machine without a GPU.  Needs the built library or the unit object files; nothing else."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import list_conv_instantiations as LI                                    # noqa: E402

LEDGER = os.path.join(ROOT, 'tests', 'golden', 'conv_instantiations.json')


def load_ledger():
    with open(LEDGER) as f:
        return json.load(f)


def test_symbol_decoder_on_hand_written_names():
    d = LI.decode_symbol
    # a kernel of namespace issk, its stub, and one of cnn.hip's unnamed namespace
    assert d('_ZN4issk17conv_x3_fp_kernelILi5ELi3ELb1ELb0ELb0ELi1EEEvNS_8ConvArgsE') == 'conv_x3_fp_kernel<5,3,true,false,false,1>'
    assert d('_ZN4issk32__device_stub__conv_x3_fp_kernelILi5ELi3ELb1ELb0ELb0ELi1EEEvNS_8ConvArgsE') is None
    assert d('_ZN12_GLOBAL__N_114conv_x3_kernelILi0ELb1ELi2EEEvN4issk8ConvArgsE') == 'conv_x3_kernel<0,true,2>'
    assert d('_ZN12_GLOBAL__N_122conv1_direct3x3_kernelILb1EEEvN4issk8ConvArgsE') == 'conv1_direct3x3_kernel<true>'
    assert d('_ZN4issk15conv_dhl_kernelILb0ELi8EEEvNS_7DhlArgsE') == 'conv_dhl_kernel<false,8>'
    # every template argument, defaults included; other integer types and negative values decode like int
    assert d('_ZN4issk17conv_x3_ws_kernelILi7ELi7ELb0ELb0ELb1ELi1ELi0ELb0ELb0ELi2EEEvNS_8ConvArgsE') == \
        'conv_x3_ws_kernel<7,7,false,false,true,1,0,false,false,2>'
    assert d('_ZN4issk15conv_toy_kernelILin3ELj12ELb1EEEvNS_8ConvArgsE') == 'conv_toy_kernel<-3,12,true>'
    # not conv kernel instantiations: other kernels, launchers, a name whose length prefix is wrong, a non-template
    assert d('_ZN4issk15resample_kernelILi4EEEvNS_7RsArgsE') is None
    assert d('_ZN4issk15launch_fp_shapeILi5ELi3EEEbRKNS_8ConvArgsE4dim3P12ihipStream_tRKNS_8ConvInstE') is None
    assert d('_ZN4issk16conv_x3_fp_kernelILi5ELi3EEEvNS_8ConvArgsE') is None
    assert d('_ZN4issk10conv_plainEv') is None
    assert d('iss_cnn_load') is None


def test_profiler_names_map_to_ledger_keys():
    c = LI.canonical_of_profiler_name
    assert c('conv_x3_fp_kernel<3,5,false,true,true,1>') == 'conv_x3_fp_kernel<3,5,false,true,true,1>'
    assert c('conv_x3_ws_kernel<5,3,false,false,true,1,1>') == 'conv_x3_ws_kernel<5,3,false,false,true,1,1,false,false,2>'
    assert c('conv_x3_ws_kernel<3,3,false,true,false,1,1,plain>') == 'conv_x3_ws_kernel<3,3,false,true,false,1,1,false,false,2>'
    assert c('conv_x3_ws_kernel<7,7,true,false,true,1,0,ring>') == 'conv_x3_ws_kernel<7,7,true,false,true,1,0,false,false,2>'
    assert c('conv_x3_ws_kernel<5,3,true,false,true,1,0,fs>') == 'conv_x3_ws_kernel<5,3,true,false,true,1,0,true,false,2>'
    assert c('conv_x3_ws_kernel<3,3,false,true,false,2,1,f32>') == 'conv_x3_ws_kernel<3,3,false,true,false,2,1,false,true,2>'
    assert c('conv_x3_ws_kernel<5,3,false,false,true,1,1,ncb1>') == 'conv_x3_ws_kernel<5,3,false,false,true,1,1,false,false,1>'
    assert c('conv_x3_pws2_kernel<true,false,dual>') == 'conv_x3_pws2_kernel<true,false,true>'
    assert c('conv_x3_pws2_kernel<true,true>') == 'conv_x3_pws2_kernel<true,true,false>'
    assert c('conv_dhl_kernel<true,8>') == 'conv_dhl_kernel<true,8>'
    for bad in ('conv_x3_ws_kernel<5,3,false,false,true,1,1,wide>', 'conv_x3_ws_kernel<5,3,false>', 'resample_kernel', 'conv_x3_pws2_kernel<true>',
                'conv_x3_fp_kernel<3,5,maybe,true,true,1>', ''):
        with pytest.raises(ValueError):
            c(bad)


@pytest.fixture(scope='module')
def held():
    paths = LI.default_paths()
    if not paths:
        pytest.skip('no built libiss_hip.so and no unit object files')
    return LI.held_instantiations(paths)


def test_ledger_equals_what_the_library_holds(held):
    ledger = load_ledger()
    assert len(held) > 100, sorted(held)                                 # (the reader found the kernels at all)
    missing = sorted(held - set(ledger))
    stale = sorted(set(ledger) - held)
    assert not missing, f'compiled instantiations without a ledger entry (add a case to tests/instantiation_cases.py): {missing}'
    assert not stale, f'ledger entries the library does not hold: {stale}'


def test_held_instantiations_and_profiler_names_are_one_to_one(held):
    names = {k: LI.profiler_name_of(k) for k in held}
    assert len(set(names.values())) == len(held)
    for key, name in names.items():
        assert LI.canonical_of_profiler_name(name) == key, (key, name)


def test_every_entry_names_a_case_or_a_clause(held):
    import instantiation_cases as IC
    for key, entry in load_ledger().items():
        if isinstance(entry, str):
            assert entry in IC.CASES, (key, entry)
        else:
            assert isinstance(entry, dict) and list(entry) == ['unreachable'], (key, entry)
            assert isinstance(entry['unreachable'], str) and len(entry['unreachable'].strip()) >= 20, (key, entry)
    used = {e for e in load_ledger().values() if isinstance(e, str)}
    assert used == set(IC.CASES), sorted(set(IC.CASES) - used)           # no case nobody points at
