"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every symbol
the headers under include/ declare.  No compute call is made (no GPU here)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(w[td]_[a-z0-9_]+)\s*\(', src)))


@pytest.fixture(scope='module')
def lib():
    from waymo_2d_tracking_amd import build
    path = build.build(verbose=False)
    return ctypes.CDLL(path)


@pytest.mark.parametrize('header', [h for h in sorted(os.listdir(os.path.join(ROOT, 'include'))) if h.endswith('.h')])
def test_every_declared_symbol_is_exported(lib, header):
    names = _declared(header)
    assert len(names) >= 5
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_abi_version_and_no_device_error(lib):
    assert lib.wt_abi_version() >= 1
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    # without a GPU the operators must fail loudly (no CPU fallback)
    n = ctypes.c_int(0)
    rc = lib.wt_device_info(ctypes.byref(n), None, 0, None)
    assert rc == 2 and n.value == 0
    lib.wt_last_error.restype = ctypes.c_char_p
    assert b'no HIP device' in lib.wt_last_error()


def test_product_never_imports_oracle():
    bad = []
    pkg = os.path.join(ROOT, 'waymo_2d_tracking_amd')
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                txt = open(os.path.join(d, f)).read()
                if re.search(r'^\s*(from|import)\s+oracle\b|wt_oracle\.h|libwt_oracle', txt, flags=re.M):
                    bad.append(f)
    assert not bad, bad


def test_split_pack_descriptor_layout_matches_the_header():
    """ops._pack_desc_dtype (the host-side array handed to wd_gemm_split_pack_batch) == struct WdSplitPackDesc of include/waymodet.h: same field order,
    offsets and size (the header is parsed, not restated)."""
    import ctypes as C
    import re
    from waymo_2d_tracking_amd.detnet.nn import ops
    text = open(os.path.join(ROOT, 'include', 'waymodet.h')).read()
    body = re.search(r'typedef struct WdSplitPackDesc \{(.*?)\} WdSplitPackDesc;', text, re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_void_p if '*' in decl else (C.c_long if decl.startswith('long') else C.c_int)
        names = decl.replace('*', ' ').split(None, 2 if decl.startswith('const') else 1)[-1]
        for name in names.split(','):
            fields.append((name.strip(), ctype))

    class Desc(C.Structure):
        _fields_ = fields

    dt = ops._pack_desc_dtype()
    assert dt.itemsize == C.sizeof(Desc) == 80
    assert [n for n, _ in fields] == list(dt.names) == list(ops._PACK_DESC_FIELDS)
    for name, _ in fields:
        assert dt.fields[name][1] == getattr(Desc, name).offset, name


def test_split_io_struct_layout_matches_the_header():
    """ops._SplitIO (handed to wd_gemm_split_io) == struct WdSplitIO of include/waymodet.h: same field names in the same order, eight 8-byte fields."""
    import ctypes as C
    import re
    from waymo_2d_tracking_amd.detnet.nn import ops
    text = open(os.path.join(ROOT, 'include', 'waymodet.h')).read()
    body = re.search(r'typedef struct WdSplitIO \{(.*?)\} WdSplitIO;', text, re.S).group(1)
    names = [d.replace('*', ' ').split()[-1] for d in body.split(';') if d.strip()]
    assert names == [f[0] for f in ops._SplitIO._fields_]
    assert C.sizeof(ops._SplitIO) == 64
    for (name, ctype), decl in zip(ops._SplitIO._fields_, [d.strip() for d in body.split(';') if d.strip()]):
        assert (ctype is C.c_long) == decl.startswith('long'), (name, decl)


def test_product_library_exports_no_laboratory_entry_points(lib):
    """Round 6: canary / occupant / burner kernels and the per-workgroup stamps live in csrc/debug/ and libwaymotrack_debug.so only."""
    for name in ('wd_debug_canary', 'wd_debug_occupy', 'wd_debug_hold', 'wd_debug_mfma_burn', 'wd_gemm_split_debug_stamps'):
        assert not hasattr(lib, name), name
    from waymo_2d_tracking_amd import build
    dbg = ctypes.CDLL(build.build_debug(verbose=False))
    assert all(hasattr(dbg, n) for n in ('wd_debug_mfma_burn', 'wd_gemm_split_debug_stamps', 'wd_gemm_split_f32'))


# Every environment variable the package reads.  A new switch is added here on purpose; a laboratory switch belongs behind
# experiment_knob() (honoured only with WT_EXPERIMENT=1), and one whose variant lost is deleted together with its code.
ENV_SWITCHES = sorted([
    'FVCORE_CACHE', 'HIPCC', 'LOCAL_RANK', 'RANK', 'WAYMO_DETECTRON2_WEIGHTS', 'WORLD_SIZE',
    'WD_CANARY_BIG', 'WD_DEBUG_BUILD', 'WD_DEBUG_FILL', 'WD_DEFORM_PATCH', 'WD_FUSED_DEFORM_BWD', 'WD_FUSED_DEFORM_DXOFF',
    'WD_FUSED_DEFORM_EPILOGUE', 'WD_FUSED_DEFORM_S2', 'WD_HIPCC_FLAGS', 'WD_SPLIT_GEMM', 'WD_SPLIT_MT', 'WD_SPLIT_NO_POSMAJOR',
    'WD_SPLIT_PLANES', 'WD_SPLIT_PLANES_MIN_CH', 'WD_SPLIT_SPLITK', 'WD_SPLIT_TRAIN',
    'WT_BENCH_INSTRUMENT_STEPS', 'WT_BENCH_NO_EXACT', 'WT_DIST_BACKEND', 'WT_EXPERIMENT', 'WT_GEMM_TUNING_ONLINE', 'WT_LIB_PATH',
    'WT_SGD_FUSED', 'WT_TUNABLEOP_IN', 'WT_TUNABLEOP_OUT', 'WT_TUNE_ITERS', 'WT_TUNE_MS',
])


def test_environment_switches_are_the_listed_ones():
    pat = re.compile(r'''\b(?:getenv|experiment_knob)\("([A-Za-z0-9_]+)"\)|\bos\.environ\.get\(['"]([A-Za-z0-9_]+)['"]''')
    found = set()
    for d, _, files in os.walk(os.path.join(ROOT, 'waymo_2d_tracking_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                found.update(a or b for a, b in pat.findall(open(os.path.join(d, f), errors='replace').read()))
    assert sorted(found) == ENV_SWITCHES


def _sources(top, suffixes=('',)):
    for d, _, files in os.walk(os.path.join(ROOT, top)):
        for f in sorted(files):
            if f.endswith(suffixes):
                yield os.path.relpath(os.path.join(d, f), ROOT), open(os.path.join(d, f), errors='replace').read()


# Every identifier a preprocessor conditional under csrc/ tests (include guards aside).  The rule above holds for these too: a compile-time
# switch whose variant lost is deleted together with its code; an experiment patches a COPY of the source (tools/split_planes_ablation_build.py).
CPP_SWITCHES = ['FB_TIMING', 'WD_DEBUG', 'WT_PHASE_TIMING', '__HIPCC__', '__cplusplus']


def test_preprocessor_switches_are_the_listed_ones():
    found = set()
    for _, txt in _sources('waymo_2d_tracking_amd/csrc', ('.hip', '.h', '.cpp')):
        # an include guard defines its name to nothing; "#ifndef X / #define X 7" is an overridable constant, i.e. a switch
        guards = set(re.findall(r'^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[ \t]*\n[ \t]*#[ \t]*define[ \t]+\1[ \t]*$', txt, flags=re.M))
        for cond in re.findall(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$', txt, flags=re.M):
            found.update(set(re.findall(r'[A-Za-z_]\w*', re.split(r'//|/\*', cond)[0])) - {'defined'} - guards)
    assert sorted(found) == CPP_SWITCHES
    # a project switch lives as long as the build or a tool compiles with it
    users = open(os.path.join(ROOT, 'waymo_2d_tracking_amd', 'build.py')).read() + ''.join(t for _, t in _sources('tools'))
    orphans = [s for s in CPP_SWITCHES if not s.startswith('__') and not re.search(r'(?:\b|-D)%s\b' % s, users)]
    assert not orphans, orphans


def test_tools_and_documents_name_only_what_the_tree_has():
    """Every tools/<path> written under tools/ or in the documents exists (a program counts when its .hip source does), and every wd_ / wt_ entry
    point a tool calls on the library is declared in include/*.h or csrc/debug/waymodet_debug.h."""
    declared = set()
    for _, txt in list(_sources('include', '.h')) + list(_sources('waymo_2d_tracking_amd/csrc/debug', '.h')):
        declared.update(re.findall(r'\b(w[td]_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', txt, flags=re.S)))
    assert len(declared) >= 100
    texts = dict(_sources('tools'))
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        texts[doc] = open(os.path.join(ROOT, doc)).read()
    missing = []
    for rel, txt in sorted(texts.items()):
        for path in sorted(set(re.findall(r'\btools/[\w./*-]*[\w*]', txt))):
            if not glob.glob(os.path.join(ROOT, path)) and not os.path.exists(os.path.join(ROOT, path + '.hip')):
                missing.append((rel, path))
        if rel.startswith('tools'):
            called = re.findall(r'\.(w[td]_[a-z0-9_]+)\s*\(|attr\(.*?,\s*[\'"](w[td]_[a-z0-9_]+)[\'"]', txt)
            missing += [(rel, name) for name in sorted({a or b for a, b in called} - declared)]
    assert not missing, missing
