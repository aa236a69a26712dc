"""Registers the compiler gives conv2's one-wave-per-SIMD kernel (conv_wq.h), from the gfx950 code object's notes: a device-only
compile of cnn_wq.hip / cnn_wq_h.hip as tools/kernel_meta.sh does it, read by tools/check_kernel_scratch.py (the build runs the
same check on every compile of these units).  The fp16 instantiations -- the segmenter nets' dominant launch -- have no scratch
and no spilled VGPR; the bf16 ones do not exceed what they had before the fp16 ones were freed of theirs
(profiles/conv2_scratch_ab.md; HIP 7.2.26015): <5,3,true,false> 18 VGPRs / 76 B, <5,3,false,false> 14 VGPRs / 56 B.  No GPU
needed; skipped without hipcc."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'inaspeechsegmenter_amd', 'csrc')
HIPCC = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
LLVM_BIN = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
TOOLS = [os.path.join(LLVM_BIN, 'clang-offload-bundler'), os.path.join(LLVM_BIN, 'llvm-readelf')]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) and all(os.path.exists(t) for t in TOOLS)),
                                reason='hipcc / the LLVM binary tools are not installed')

WQ = '_ZN4issk17conv_x3_wq_kernelILi5ELi3ELb%dELb%dEEEvNS_8ConvArgsE'      # <5, 3, OUT_HL, F16>


def _checker():
    spec = importlib.util.spec_from_file_location('check_kernel_scratch', os.path.join(ROOT, 'tools', 'check_kernel_scratch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _notes(unit, tmp):
    """{kernel: figures} of one unit, compiled for the device only with the build's flags."""
    bundle, elf = os.path.join(tmp, unit + '.bundle'), os.path.join(tmp, unit + '.elf')
    subprocess.run([HIPCC, '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '--offload-arch=gfx950', '-Wno-unused-function',
                    '-mllvm', '-pragma-unroll-threshold=100000', '-I../../include', '--cuda-device-only', '-c', unit + '.hip',
                    '-o', bundle], cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([TOOLS[0], '--unbundle', '--type=o', '--input=' + bundle, '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                    '--output=' + elf], check=True)
    text = subprocess.run([TOOLS[1], '--notes', elf], check=True, capture_output=True, text=True).stdout
    return _checker().parse_notes(text)


def test_fp16_conv2_has_no_scratch(tmp_path):
    k = _notes('cnn_wq_h', str(tmp_path))
    for hl in (1, 0):
        fig = k[WQ % (hl, 1)]
        print(WQ % (hl, 1), fig)
        assert fig['private_segment_fixed_size'] == 0 and fig['vgpr_spill_count'] == 0, fig
        assert fig['agpr_count'] == 256 and fig['group_segment_fixed_size'] == 160 * 1024, fig       # still the kernel it was


def test_bf16_conv2_no_worse_than_before(tmp_path):
    k = _notes('cnn_wq', str(tmp_path))
    for hl, vgprs, scratch in ((1, 18, 76), (0, 14, 56)):
        fig = k[WQ % (hl, 0)]
        print(WQ % (hl, 0), fig)
        assert fig['vgpr_spill_count'] <= vgprs and fig['private_segment_fixed_size'] <= scratch, fig


def test_notes_parser_reads_every_kernel():
    """The parser on a hand-written notes text: nested argument entries and list items do not end or rename a kernel."""
    text = '\n'.join([
        'amdhsa.kernels:',
        '  - .agpr_count:     256',
        '    .args:',
        '      - .name:           p',
        '        .offset:         0',
        '    .language_version:',
        '      - 2',
        '      - 0',
        '    .name:           k_one',
        '    .private_segment_fixed_size: 76',
        '    .sgpr_spill_count: 117',
        '    .vgpr_count:     512',
        '    .vgpr_spill_count: 18',
        '  - .agpr_count:     0',
        '    .name:           k_two',
        '    .private_segment_fixed_size: 0',
        '    .vgpr_spill_count: 0',
        'amdhsa.target:   amdgcn-amd-amdhsa--gfx950',
        '    .name:           not_a_kernel'])
    k = _checker().parse_notes(text)
    assert set(k) == {'k_one', 'k_two'}
    assert k['k_one'] == {'agpr_count': 256, 'private_segment_fixed_size': 76, 'sgpr_spill_count': 117, 'vgpr_count': 512, 'vgpr_spill_count': 18}
    assert k['k_two']['private_segment_fixed_size'] == 0
