"""CPU checks of the PIL-exact bilinear resize: the host tables of the library against a Python restatement, the CPU form of the whole
resize against the installed PIL on every case, the case classes, the refusals, and the --resize argument parsing.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from resize_cases import CLASSES, CLASS_CHECKS, CONTENTS, MAX_SIZE, SHAPES, class_facts, ksize, make_image, pil_resize, resize_ref, shape_id, tables


@pytest.fixture(scope='module')
def lib():
    from waymo_2d_tracking_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _last_error(lib):
    return lib.wt_last_error().decode()


def _host_tables(lib, n_in, n_out):
    ks = lib.wd_resize_ksize(C.c_int(n_in), C.c_int(n_out))
    bounds = np.full((n_out, 2), -1, np.int32)
    coeffs = np.full((n_out, max(ks, 1)), -1, np.int32)
    rc = lib.wd_resize_tables_host(C.c_int(n_in), C.c_int(n_out), bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p))
    return rc, ks, bounds, coeffs


def _host_resize(lib, img, oh, ow):
    img = np.ascontiguousarray(img)
    out = np.full((oh, ow, 3), 0x5A, np.uint8)
    rc = lib.wd_resize_bilinear_u8_host(img.ctypes.data_as(C.c_void_p), C.c_int(img.shape[0]), C.c_int(img.shape[1]),
                                        out.ctypes.data_as(C.c_void_p), C.c_int(oh), C.c_int(ow))
    assert rc == 0, _last_error(lib)
    return out


AXES = sorted({(s[0][a], s[1][a]) for s in SHAPES for a in (0, 1) if s[0][a] != s[1][a]} | {(1280, 800), (1920, 1200)})


@pytest.mark.parametrize('n_in,n_out', AXES, ids=['%d-%d' % a for a in AXES])
def test_host_tables_equal_the_restated_definition(lib, n_in, n_out):
    rc, ks, bounds, coeffs = _host_tables(lib, n_in, n_out)
    assert rc == 0, _last_error(lib)
    exp_bounds, exp_coeffs = tables(n_in, n_out)
    assert ks == ksize(n_in, n_out) == exp_coeffs.shape[1]
    assert np.array_equal(bounds, exp_bounds)
    assert np.array_equal(coeffs, exp_coeffs)                      # entry for entry, the zeros behind count included
    assert int(coeffs.sum(1).max()) * 255 < 2 ** 31


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_host_resize_equals_pil(lib, shape, content):
    img = make_image(shape, content)
    oh, ow = shape[1]
    exp = pil_resize(img, oh, ow)
    got = _host_resize(lib, img, oh, ow)
    assert np.array_equal(got, exp), '%d of %d bytes differ' % (int((got != exp).sum()), exp.size)
    assert np.array_equal(resize_ref(img, oh, ow), exp)           # the restatement the class checks are built on is PIL's too
    if content == 'full':
        assert int(got.min()) == 255
    if content == 'zeros':
        assert int(got.max()) == 0


def test_host_resize_equals_pil_on_a_full_size_frame(lib):
    img = np.random.default_rng(5).integers(0, 256, (1280, 1920, 3), dtype=np.uint8)
    assert np.array_equal(_host_resize(lib, img, 800, 1200), pil_resize(img, 800, 1200))


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_every_case_is_in_its_class(name):
    for shape in CLASSES[name]:
        facts = class_facts(shape)
        assert CLASS_CHECKS[name](facts, shape), (name, shape, facts)
        for axis, a in ((1, 'x'), (0, 'y')):
            f = facts[a]
            assert f['skipped'] == (shape[0][axis] == shape[1][axis])
            if f['skipped']:
                continue
            # the last window always reaches past the source and is cut at in_size; the first one is cut at 0 once scale >= 3
            assert f['clamped_high'], (shape, a)
            assert f['clamped_low'] == (shape[0][axis] / shape[1][axis] >= 3), (shape, a)
            assert f['sum_offsets'] <= set(range(-4, 5)), f['sum_offsets']


def test_the_cases_cover_both_clamps_both_skips_and_an_inexact_row_sum():
    facts = [class_facts(s) for s in SHAPES]
    axes = [f[a] for f in facts for a in 'xy']
    assert any(a['clamped_low'] for a in axes) and any(a['clamped_high'] for a in axes)
    assert any(f['x']['skipped'] and not f['y']['skipped'] for f in facts)
    assert any(f['y']['skipped'] and not f['x']['skipped'] for f in facts)
    assert any(f['x']['skipped'] and f['y']['skipped'] for f in facts)
    # found, not assumed: the (128, 192) -> (80, 120) tables hold a row whose weights do not sum to 2^22
    offsets = class_facts(CLASSES['row_sum'][0])
    assert (offsets['x']['sum_offsets'] | offsets['y']['sum_offsets']) - {0}
    assert {35, 301, 5, 3} <= {a['ksize'] for a in axes}


@pytest.mark.parametrize('n_in,n_out,word', [(0, 4, 'in_size = 0'), (4, 0, 'out_size = 0'), (MAX_SIZE + 1, 4, 'in_size = 16385'),
                                               (4, MAX_SIZE + 1, 'out_size = 16385'), (-3, 4, 'in_size = -3')])
def test_tables_refuse_bad_sizes_by_name(lib, n_in, n_out, word):
    assert lib.wd_resize_ksize(C.c_int(n_in), C.c_int(n_out)) == 0
    buf = np.zeros(64, np.int32)
    rc = lib.wd_resize_tables_host(C.c_int(n_in), C.c_int(n_out), buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))
    assert rc == 1 and word in _last_error(lib), _last_error(lib)


def test_tables_refuse_null_pointers_by_name(lib):
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.wd_resize_tables_host(C.c_int(4), C.c_int(2), None, p) == 1 and 'bounds is null' in _last_error(lib)
    assert lib.wd_resize_tables_host(C.c_int(4), C.c_int(2), p, None) == 1 and 'coeffs is null' in _last_error(lib)


@pytest.mark.parametrize('h,w,oh,ow,word', [(0, 4, 2, 2, 'h = 0'), (4, 0, 2, 2, 'w = 0'), (4, 4, 0, 2, 'oh = 0'), (4, 4, 2, 0, 'ow = 0'),
                                             (MAX_SIZE + 1, 4, 2, 2, 'h = 16385'), (4, 4, 2, MAX_SIZE + 1, 'ow = 16385')])
def test_resize_refuses_bad_sizes_by_name(lib, h, w, oh, ow, word):
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.wd_resize_bilinear_u8_workspace(C.c_int(h), C.c_int(w), C.c_int(oh), C.c_int(ow)) == 0
    for fn, extra in ((lib.wd_resize_bilinear_u8_host, ()), (lib.wd_resize_bilinear_u8, (p, p, p, p, p, C.c_size_t(64), None))):
        rc = fn(p, C.c_int(h), C.c_int(w), p, C.c_int(oh), C.c_int(ow), *extra)
        assert rc == 1 and word in _last_error(lib), _last_error(lib)      # refused on the host, before a device is looked for


def test_resize_refuses_null_pointers_by_name(lib):
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    four = [C.c_int(4)] * 2
    assert lib.wd_resize_bilinear_u8_host(None, *four, p, C.c_int(2), C.c_int(2)) == 1 and 'src is null' in _last_error(lib)
    assert lib.wd_resize_bilinear_u8_host(p, *four, None, C.c_int(2), C.c_int(2)) == 1 and 'dst is null' in _last_error(lib)
    tail = (p, C.c_size_t(64), None)
    assert lib.wd_resize_bilinear_u8(p, *four, p, C.c_int(2), C.c_int(2), None, p, p, p, *tail) == 1 and 'xbounds is null' in _last_error(lib)
    assert lib.wd_resize_bilinear_u8(p, *four, p, C.c_int(2), C.c_int(2), p, p, p, None, *tail) == 1 and 'ycoeffs is null' in _last_error(lib)
    assert lib.wd_resize_bilinear_u8(p, *four, p, C.c_int(2), C.c_int(2), p, p, p, p, None, C.c_size_t(64), None) == 1
    assert 'workspace is null' in _last_error(lib)
    # the intermediate of 4x4 -> 2x2 is 4 * 2 * 3 bytes: one byte short is a capacity error, and none is needed for one pass
    assert lib.wd_resize_bilinear_u8_workspace(*four, C.c_int(2), C.c_int(2)) == 24
    assert lib.wd_resize_bilinear_u8_workspace(*four, C.c_int(4), C.c_int(2)) == 0
    assert lib.wd_resize_bilinear_u8(p, *four, p, C.c_int(2), C.c_int(2), p, p, p, p, p, C.c_size_t(23), None) == 4
    assert 'workspace_bytes = 23' in _last_error(lib)


def _parse(*argv):
    from waymo_2d_tracking_amd.detnet import inference as I
    args = I.build_parser().parse_args(['-i', 'x', '--export', 'y.json'] + list(argv))
    I.check_supported(args)
    return I.parse_resize(args)


def test_resize_argument_parsing():
    assert _parse('--resize', '300x200', '--resize-device', 'gpu') == (200, 300)          # WxH -> (h, w), like the reference
    assert _parse('--resize', '800', '--resize-device', 'gpu') == 800
    assert _parse('--resize', '800') == 800
    assert _parse() is None
    with pytest.raises(NotImplementedError):
        _parse('--resize', '300x200')
    with pytest.raises(NotImplementedError):
        _parse('--resize', '300x200', '--resize-device', 'host')
    with pytest.raises(ValueError):
        _parse('--resize', '300x200', '--resize-device', 'gpu', '--max-image-size', '256')
    assert _parse('--resize', '300', '--max-image-size', '256') == 300
    with pytest.raises(ValueError):
        _parse('--resize', '300x', '--resize-device', 'gpu')
