"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/salsa_hip.h declares, and its host
helpers (bin limits, compression matrix) agree with the reference goldens.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'salsa_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = set(re.findall(r'\b(salsa_[a-z_]+)\s*\(', hdr))
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), 'libsalsa_hip.so does not export %s' % n
    from salsa_amd import _lib
    assert set(_lib.EXPORTS) == names
    assert lib.salsa_abi_version() == 2
    gru = open(os.path.join(ROOT, 'include', 'salsa_gru.h')).read()
    gru = re.sub(r'/\*.*?\*/', '', gru, flags=re.S)
    gnames = set(re.findall(r'\b(salsa_gru_[a-z_]+)\s*\(', gru))
    assert gnames == set(_lib.GRU_EXPORTS) and all(hasattr(lib, n) for n in gnames)
    lnames = set(re.findall(r'\b(salsa_lstm_[a-z_]+)\s*\(', gru))
    assert lnames == set(_lib.LSTM_EXPORTS) and all(hasattr(lib, n) for n in lnames)
    nn = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_nn.h')).read(), flags=re.S)
    nnames = set(re.findall(r'\b(salsa_nn_[a-z0-9_]+)\s*\(', nn))
    assert nnames == set(_lib.NN_EXPORTS) and all(hasattr(lib, n) for n in nnames)
    base = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_baseline.h')).read(), flags=re.S)
    bnames = set(re.findall(r'\b(salsa_baseline_[a-z_]+)\s*\(', base))
    assert bnames == set(_lib.BASELINE_EXPORTS) and all(hasattr(lib, n) for n in bnames)
    # the header parser that binds the library sees exactly these, each once: nothing is skipped, nothing invented
    every = names | gnames | lnames | nnames | bnames
    parsed = {n: v for h in _lib.HEADERS for n, v in _lib.PROTOTYPES[h].items()}
    assert len(every) >= 104 and set(parsed) == every and sum(len(_lib.PROTOTYPES[h]) for h in _lib.HEADERS) == len(every)
    for n, (restype, argtypes) in parsed.items():                # ... and load() bound each of them as parsed
        assert getattr(lib, n).restype is restype and list(getattr(lib, n).argtypes) == argtypes, n


def test_parsed_signatures_match_hand_written_ones(lib):
    """The binding is derived from include/*.h (salsa_amd/_lib.py parse_prototypes); these ten are spelled out by hand from the headers
    and cover every kind of its table: int / int64_t / size_t / float / double / uint32_t parameters, data, struct, plan and
    pointer-to-pointer parameters, int / int64_t / size_t / const char * returns, and (void)."""
    vp, i, i64, sz, f, d, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float, C.c_double, C.c_uint32
    want = {
        'salsa_nn_bn_train_fwd_bits': (i, [vp, vp, vp, i, i64, i, vp, vp, f, f, vp, vp, vp, vp, vp, i, f, u32, vp, vp, i, vp, vp]),
        'salsa_nn_adam_step': (i, [vp, vp, i, vp, i, d, d, d, d, d, i64, vp]),
        'salsa_resample_batch': (i, [vp, i, i64, vp, i64, i64, d, vp, vp, i, i, vp, vp]),
        'salsa_workspace_bytes': (sz, [vp, i, i64]),
        'salsa_nn_conv3x3_wide_table_len': (i64, [i64, i, i]),
        'salsa_last_error': (C.c_char_p, []),
        'salsa_nn_get_deterministic': (i, []),
        'salsa_plan_read_timing': (i, [vp, vp, vp, vp]),
        'salsa_nn_seld_score': (i, [vp, vp, i, vp, vp, i, i, i, i, i, d, d, vp, vp, vp, vp, vp, vp]),
        'salsa_baseline_mel_matrix': (i, [i, i, i, d, d, vp]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_parser_refuses_a_type_outside_its_table():
    from salsa_amd import _lib
    ok = _lib.parse_prototypes('/* c */\n#define X 1\nsize_t salsa_fine(const int64_t n, const char **names, float);\n')
    assert ok == {'salsa_fine': (C.c_size_t, [C.c_int64, C.c_void_p, C.c_float])}
    for bad in ('int salsa_made_up(int n, long double x);', 'int salsa_made_up(unsigned short n, float *p);', 'int salsa_made_up(salsa_params p);',
                'float *salsa_made_up(int n);', 'void salsa_made_up(int n);', 'unsigned salsa_made_up(void);',
                'int salsa_made_up(int (*callback)(int), void *user);'):
        with pytest.raises(TypeError, match='salsa_made_up'):
            _lib.parse_prototypes('int salsa_before(int a);\n' + bad + '\nint salsa_after(void);\n')


def test_one_source_list():
    """Every salsa_amd/csrc/*.hip is compiled by the product's build, in sorted order, and nothing from elsewhere is."""
    from salsa_amd import _lib
    csrc = os.path.join(ROOT, 'salsa_amd', 'csrc')
    hips = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.hip'))
    cmd = _lib.build_command()
    assert len(hips) >= 10 and [a for a in cmd if a.endswith('.hip')] == hips
    assert [a for a in cmd if os.sep in a and a not in hips] == [_lib.LIB_PATH]


def test_host_helpers_match_reference(lib):
    from salsa_amd.extractor import bin_limits, compress_matrix
    meta, a = load_golden('g5_w_bins')
    for fs, n_fft, fmin, fmax, lo, up, cut in meta['bins']:
        assert bin_limits(fs, n_fft, fmin, fmax) == (lo, up, cut)
    for n_fft in (512, 256):
        for comp, tag in ((True, 'c'), (False, 'n')):
            assert np.array_equal(compress_matrix(n_fft, comp), a['W_%d_%s' % (n_fft, tag)])
    with pytest.raises(AssertionError):
        compress_matrix(1024)


def test_params_struct_layout_matches_header():
    from salsa_amd import _lib
    # 6 ints, double (8-aligned), 7 ints, pad -> 64 bytes with natural alignment
    assert C.sizeof(_lib.SalsaParams) == 80
    assert _lib.SalsaParams.cond_num.offset == 24


def test_probe_switches_are_quarantined_and_the_default_build_says_so(lib, tmp_path):
    """Round-5 review, item 7: ~37 timing-probe switches (most of them wrong-result on purpose) and ~68 tunables live in the
    production translation units.  (1) salsa_amd/csrc/build_guard.h -- generated, checked here to be current -- makes any probe
    switch a compile ERROR unless -DSALSA_PROBE_BUILD is given too; (2) the product's build command carries no -D at all;
    (3) the library says what it was built with: salsa_build_flags() is empty for the product."""
    import subprocess
    import sys
    from salsa_amd import _lib
    gen = os.path.join(ROOT, 'tools', 'gen_build_guard.py')
    assert subprocess.run([sys.executable, gen, '--check']).returncode == 0, 'build_guard.h is stale: python tools/gen_build_guard.py'
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_build_guard
    switches, tunables = gen_build_guard.scan()
    assert {'CONV_ZERO_SRC', 'CONV_PROBE_ROLL', 'CONV_FETCH_COLMAJOR', 'WIDE_X_ZERO', 'TR_PROBE_NO_CONSUME', 'FZ_PROBE_NOSOLVE',
            'GRU_PROBE_BWD_NO_LOAD', 'BN_PROBE_NO_Y', 'STEM_NO_STORE'} <= set(switches)
    assert {'K1_SPILL_NT', 'K3_OUT_NT', 'K3_FT_N', 'SALSA_PK_GATE_TOL', 'CONV_RES_EARLY'} <= set(tunables)
    csrc = os.path.join(ROOT, 'salsa_amd', 'csrc')
    for f in os.listdir(csrc):                                   # every translation unit starts from the guard
        if f.endswith('.hip'):
            assert '#include "build_guard.h"' in open(os.path.join(csrc, f)).read(), f
    assert not [a for a in _lib.build_command() if a.startswith('-D')]
    assert lib.salsa_build_flags() == b'' and _lib.build_flags() == ''
    # the guard itself (plain preprocessor: g++ suffices): a probe switch alone is refused, with the marker it is admitted and named
    tu = tmp_path / 'tu.cpp'
    tu.write_text('#include "build_guard.h"\nconst char *flags = SALSA_BUILD_FLAGS;\n#include <stdio.h>\nint main() { puts(flags); return 0; }\n')
    exe = str(tmp_path / 'tu')
    base = ['g++', '-I', csrc, str(tu), '-o', exe]
    for sw in ('CONV_ZERO_SRC', 'TR_PROBE_NO_CONSUME', 'K1_FRAME_MAJOR'):
        r = subprocess.run(base + ['-D' + sw], capture_output=True, text=True)
        assert r.returncode != 0 and 'SALSA_PROBE_BUILD' in r.stderr, sw
    assert subprocess.run(base, capture_output=True).returncode == 0
    assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == ''
    assert subprocess.run(base + ['-DCONV_ZERO_SRC', '-DSALSA_PROBE_BUILD', '-DK3_FT_N=16'], capture_output=True).returncode == 0
    assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == 'PROBE K3_FT_N=16'


def test_hand_issued_residual_loads_are_not_touched_before_their_wait():
    """Round-5 advisor (medium): conv_mfma.hip's early residual loads are bare asm global loads the compiler cannot see as in flight;
    only its register allocation keeps a copy / spill away from their destination registers until the counted wait.  The ISA of
    every build is checked (tools/asm_async_loads.py); the checker itself is checked on two synthetic listings."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import asm_async_loads as chk
    n, bad = chk.check(os.path.join(ROOT, 'salsa_amd', 'csrc', 'conv_mfma.hip'))
    assert n >= 8 and not bad, bad
    good = ['_Zk:', ';;#ASMSTART', 'global_load_dwordx2 v[10:11], v[2:3], off', ';;#ASMEND', 'v_mfma_f32_32x32x16_bf16 a[0:15], v[4:7], v[8:9], a[0:15]',
            's_waitcnt vmcnt(2)', 'v_pk_add_f32 v[20:21], v[10:11], v[12:13]', '.Lfunc_end0:']
    assert chk.check_lines(good) == (1, [])
    for touch in ('v_mov_b32_e32 v40, v10', 'scratch_store_dwordx2 off, v[10:11], s32 offset:16', 'v_add_f32_e32 v11, v1, v2'):
        n, bad = chk.check_lines(good[:5] + [touch] + good[5:])
        assert n == 1 and len(bad) == 1 and bad[0][4] == touch


def test_shared_kernel_helpers_are_defined_once():
    """The bf16 helpers were once copied by hand into four units.  pack_bf16 (the rounding every bf16 store shares) and bf2f each have ONE
    definition among the sources, and tr_frag -- the transposing LDS read's fragment -- is defined by no unit: conv_c64_wrw.hip,
    conv_stem_wrw.hip and conv_1x1.hip all take conv_internal.h's."""
    csrc = os.path.join(ROOT, 'salsa_amd', 'csrc')
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    for name, home in (('pack_bf16', 'nn_common.h'), ('bf2f', 'nn_vec.h')):
        definition = re.compile(r'^[ \t]*(?:[\w*&:<>]+[ \t]+)+[*&]?%s[ \t]*\([^;()]*\)[ \t]*(?://.*)?\n?[ \t]*\{' % name, re.M)   # `type name(params) {`
        assert [f for f, t in text.items() if definition.search(t)] == [home], name
        assert sum(len(definition.findall(t)) for t in text.values()) == 1, name
        assert sum(len(re.findall(r'\b%s\s*\(' % name, t)) for t in text.values()) > 1, name      # ... and it is called
    assert [f for f, t in text.items() if re.search(r'\bstruct\s+tr_frag\b[^;]*\{', t)] == ['conv_internal.h']
