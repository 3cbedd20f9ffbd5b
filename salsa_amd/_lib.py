"""ctypes binding of libsalsa_hip.so (C ABI in include/salsa_hip.h).  There is no CPU fallback: if the HIP library
is missing this module raises, loudly, with the build command."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SALSA_HIP_LIB') or os.path.join(_HERE, 'lib', 'libsalsa_hip.so')   # (env override: A/B probes of kernel variants)
CSRC_DIR = os.path.join(_HERE, 'csrc')          # every *.hip in it is a translation unit of the library (build_command)
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), 'include')
HEADERS = ('salsa_hip.h', 'salsa_gru.h', 'salsa_nn.h', 'salsa_baseline.h')

FORMAT = {'foa': 0, 'mic': 1}
FEATURE = {'salsa': 0, 'salsa_lite': 1, 'salsa_ipd': 2}
LAYOUT = {'planar': 0, 'interleaved': 1}
BANK_RECIPE = {'none': 0, 'foa': 1, 'mic': 2, 'gcc': 3}   # salsa_bank_batch: SALSA_BANK_*
FLAG_FLEX, FLAG_NO_CLIP_FREQS, FLAG_CLIP_SPATIAL_ALIAS = 1, 2, 4
FLAG_FORCE_F64 = 8  # verification: the all-float64 instantiation of the covariance / eigen kernel (include/salsa_hip.h)
PIPE_SPLIT_PAIRS, PIPE_GRAPH = 1, 2
MAX_KERNELS = 32

PARTIAL = 1     # salsa_extract_batch in the prefix-issue measurement mode (include/salsa_hip.h: SALSA_PARTIAL)
E_INVAL, E_NFFT, E_FORMAT, E_BINS, E_WORKSPACE, E_HIP = -1, -2, -3, -4, -5, -6


class SalsaParams(C.Structure):
    _fields_ = [('fs', C.c_int), ('n_fft', C.c_int), ('hop_len', C.c_int), ('win_len', C.c_int),
                ('fmin_doa', C.c_int), ('fmax_doa', C.c_int), ('cond_num', C.c_double), ('n_hopframes', C.c_int),
                ('is_tracking', C.c_int), ('is_compress_high_freq', C.c_int), ('audio_format', C.c_int),
                ('feature_type', C.c_int), ('audio_layout', C.c_int), ('flags', C.c_int),
                ('floor_mask_ratio', C.c_double), ('fmax_spec', C.c_int), ('reserved', C.c_int)]


# include/salsa_baseline.h
BASELINE_FEATURE = {'melspec': 0, 'melspeciv': 1, 'melspecgcc': 2, 'linspeciv': 3, 'linspecgcc': 4}


class BaselineParams(C.Structure):
    _fields_ = [('fs', C.c_int), ('n_fft', C.c_int), ('hop_len', C.c_int), ('win_len', C.c_int), ('n_mels', C.c_int),
                ('feature_type', C.c_int), ('fmin', C.c_double), ('fmax', C.c_double), ('is_compressed_freq', C.c_int),
                ('reserved', C.c_int)]


_lib = None


def build_command():
    return (['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC', '-o', LIB_PATH]
            + sorted(os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith('.hip')))


_CTYPES = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'float': C.c_float, 'double': C.c_double, 'uint32_t': C.c_uint32}


def _ctype(decl, named, proto):
    words = [w for w in decl.split() if w != 'const']
    key = ' '.join(words[:-1] if named and len(words) > 1 else words)
    if key not in _CTYPES:
        raise TypeError('no ctypes mapping for "%s" in `%s`' % (' '.join(decl.split()), proto))
    return _CTYPES[key]


def parse_prototypes(text):
    """{name: (restype, argtypes)} of every `ret salsa_name(args);` prototype of a C header's text, in its order.  One rule per kind: the
    scalars of _CTYPES, any pointer parameter -> c_void_p, a `const char *` return -> c_char_p, `(void)` -> [].  A prototype this cannot
    read, or a type outside the table, raises and names the function: nothing is skipped or bound as int by default."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r'([^;{}()]*?)\b(salsa_\w+)\s*\(([^()]*)\)\s*;', text):
        proto = ' '.join(('%s %s(%s)' % (ret, name, args)).split())
        restype = C.c_char_p if ret.split() == ['const', 'char', '*'] else _ctype(ret, False, proto)
        params = [] if args.split() == ['void'] else args.split(',')
        protos[name] = (restype, [C.c_void_p if '*' in a else _ctype(a, True, proto) for a in params])
    declared = re.findall(r'\b(salsa_\w+)\s*\(', text)
    if declared != list(protos):
        raise TypeError('unreadable prototype of %s' % sorted(set(declared) ^ set(protos)))
    return protos


PROTOTYPES = {h: parse_prototypes(open(os.path.join(INCLUDE_DIR, h)).read()) for h in HEADERS}      # the only registration of an entry point
EXPORTS = list(PROTOTYPES['salsa_hip.h'])
GRU_EXPORTS = [n for n in PROTOTYPES['salsa_gru.h'] if n.startswith('salsa_gru_')]
LSTM_EXPORTS = [n for n in PROTOTYPES['salsa_gru.h'] if n.startswith('salsa_lstm_')]
NN_EXPORTS = list(PROTOTYPES['salsa_nn.h'])
BASELINE_EXPORTS = list(PROTOTYPES['salsa_baseline.h'])


def load():
    """Load libsalsa_hip.so; raise if it has not been built (the product never falls back to CPU code)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libsalsa_hip.so is missing (%s). Build it with `python -c "import __graft_entry__ as g; '
                           'g.build()"` or: %s' % (LIB_PATH, ' '.join(build_command())))
    L = C.CDLL(LIB_PATH)
    for protos in PROTOTYPES.values():                # a library without one of them fails to load here: build() with it
        for name, (restype, argtypes) in protos.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    flags = L.salsa_build_flags().decode()
    if flags:                                        # an A/B or probe library (SALSA_HIP_LIB / tools/dev_build.sh with -D...): say so, loudly
        import sys
        sys.stderr.write('salsa_amd: %s was NOT built with the product\'s flags:%s%s\n'
                         % (LIB_PATH, flags, ' -- a PROBE build computes wrong results on purpose' if ' PROBE' in flags else ''))
    _lib = L
    return L


def build_flags() -> str:
    """'' for the product's build; otherwise the probe marker / overridden tunables the loaded library reports (salsa_build_flags)."""
    return load().salsa_build_flags().decode()


def last_error() -> str:
    return load().salsa_last_error().decode()

