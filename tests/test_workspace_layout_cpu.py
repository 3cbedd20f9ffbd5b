"""CPU tests of the extractor's workspace layout (salsa_amd/csrc/salsa_workspace.h, compiled by g++ through tests/hostemu/workspace_emu.cpp):
regions aligned, ordered and disjoint; totals equal to the formulas the three *_workspace_bytes queries have always returned, restated
here, for both mask sizings; a clip group offset by exactly its first clip's strides and ending inside its region; and the same table
walked by a stand-alone program under AddressSanitizer / UBSan, every group writing its share of a buffer of exactly `total` bytes."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, 'tests', 'hostemu', 'workspace_emu.cpp')
FIELDS = ('spill_off', 'spill_bytes', 'gate_off', 'gate_bytes', 'doubt_off', 'doubt_bytes', 'flag_off', 'flag_bytes', 'total',
          'spill_clip', 'mask_clip', 'flag_clip')
# (batch, T, nd, nch, tight): the 4-channel entry points size their masks in whole chunks, the N-microphone path tightly
SHAPES = [(b, T, nd, nch, tight) for nd in (1, 33, 64, 65, 191) for T in (1, 63, 64, 65, 161) for b in (1, 5)
          for nch, tight in ((4, 0), (6, 1), (16, 1))]


def align256(x):
    return (x + 255) & ~255


def total_four(b, T, nd):
    """salsa_workspace_bytes / salsa_eigvec_workspace_bytes: spill, gate masks, doubt mask, doubt flags, 256 spare"""
    mask = align256(b * ((T + 63) // 64) * ((nd + 63) // 64) * 64 * 8)
    return align256(b * T * 4 * nd * 8) + 2 * mask + align256(4 * b) + 256


def total_multi(b, T, nd, nch):
    """salsa_multichannel_workspace_bytes: spill, one tightly sized gate mask, 256 spare"""
    return align256(b * T * nch * nd * 8) + align256(b * ((nd + 31) // 32) * T * 4) + 256


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('workspace_emu') / 'libworkspace_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, EMU_SRC])
    L = C.CDLL(so)
    L.emu_workspace_layout.restype = None
    L.emu_workspace_layout.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.emu_workspace_group.restype = None
    L.emu_workspace_group.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    return L


def layout(emu, shape):
    out = (C.c_uint64 * len(FIELDS))()
    emu.emu_workspace_layout(*shape, out)
    return dict(zip(FIELDS, out))


def test_source_is_plain_cxx():
    """the header is the host compiler's to build: no HIP include, and the emulation includes nothing else of the library"""
    header = open(os.path.join(ROOT, 'salsa_amd', 'csrc', 'salsa_workspace.h')).read()
    assert 'hip' not in [ln.split()[1].strip('<>"').split('/')[0] for ln in header.splitlines() if ln.startswith('#include')]
    includes = [ln.split()[1] for ln in open(EMU_SRC).read().splitlines() if ln.startswith('#include "')]
    assert includes == ['"../../salsa_amd/csrc/salsa_workspace.h"']


def test_regions_are_aligned_ordered_and_disjoint(emu):
    for shape in SHAPES:
        L = layout(emu, shape)
        end = 0
        for r in ('spill', 'gate', 'doubt', 'flag'):
            off, size = L[r + '_off'], L[r + '_bytes']
            assert off % 256 == 0 and size % 256 == 0, (shape, r)
            assert off >= end, (shape, r)                                  # in order, and past the end of the region before
            end = off + size
        assert end <= L['total'], shape
        if shape[4]:
            assert L['doubt_bytes'] == 0 and L['flag_bytes'] == 0, shape     # the N-microphone path has gate masks only


def test_totals_are_the_queries_formulas(emu):
    for b, T, nd, nch, tight in SHAPES:
        want = total_multi(b, T, nd, nch) if tight else total_four(b, T, nd)
        assert layout(emu, (b, T, nd, nch, tight))['total'] == want, (b, T, nd, nch, tight)
    # the eigvec entry points pass bins and frames of their own: the same layout, any size
    for b, T, nd in itertools.product((1, 3), (7, 130), (2, 200)):
        assert layout(emu, (b, T, nd, 4, 0))['total'] == total_four(b, T, nd)


def test_per_clip_strides_are_what_the_kernels_index(emu):
    """spectra [t][pair][bin] float4 = T * nch * nd complex64; a mask [32-bin group][t] uint32, tightly; one flag word"""
    for b, T, nd, nch, tight in SHAPES:
        L = layout(emu, (b, T, nd, nch, tight))
        assert (L['spill_clip'], L['mask_clip'], L['flag_clip']) == (T * nch * nd * 8, ((nd + 31) // 32) * T * 4, 4)


def test_a_group_is_offset_by_its_first_clip_and_stays_inside(emu):
    out = (C.c_uint64 * 5)()
    for shape in SHAPES:
        b = shape[0]
        L = layout(emu, shape)
        for G in (1, 2, 3):
            G = min(G, b)
            for g in range(G):
                g0, g1 = b * g // G, b * (g + 1) // G                       # the schedule's split: uneven for 5 clips
                emu.emu_workspace_group(*shape, g0, g1 - g0, out)
                assert out[0] == L['spill_off'] + g0 * L['spill_clip'] and out[4] == (g1 - g0) * L['spill_clip'], (shape, g0)
                assert out[1] == L['gate_off'] + g0 * L['mask_clip'] and out[2] == L['doubt_off'] + g0 * L['mask_clip'], (shape, g0)
                assert out[3] == L['flag_off'] + g0 * L['flag_clip'], (shape, g0)
                # the group's last element lies inside its region (the last group of the split reaches furthest)
                assert out[0] + out[4] <= L['spill_off'] + L['spill_bytes'], (shape, g0)
                assert out[1] + (g1 - g0) * L['mask_clip'] <= L['gate_off'] + L['gate_bytes'], (shape, g0)
                if not shape[4]:
                    assert out[2] + (g1 - g0) * L['mask_clip'] <= L['doubt_off'] + L['doubt_bytes'], (shape, g0)
                    assert out[3] + L['flag_clip'] <= L['flag_off'] + L['flag_bytes'], (shape, g0)
            assert g1 == b


def test_sanitizer_program_runs_clean(tmp_path):
    """the stand-alone program (its own main, nothing loaded into python): AddressSanitizer + UBSan while every group of 1-, 2-, 3- and
    8-way splits writes its share of each region into an allocation of exactly `total` bytes"""
    exe = str(tmp_path / 'workspace_emu')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-o', exe, EMU_SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'all layouts clean' in r.stdout, r.stdout + r.stderr
