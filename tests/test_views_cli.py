"""CPU checks of the inference CLI's --views flags: parsing, weight normalisation, unfoldable specs and conflicting flags."""
import pytest

from waymo_2d_tracking_amd.detnet import inference as I


def _args(*argv):
    return I.build_parser().parse_args(['-i', 'imgs', '--export', 'm.json'] + list(argv))


def test_views_are_parsed_into_tta_token_lists():
    specs, views, weights = I.check_views(_args('--views', 'orig;x1.2; x1.5,hflip'))
    assert specs == ['orig', 'x1.2', 'x1.5,hflip']
    assert views == [['orig'], ['x1.2'], ['x1.5', 'hflip']]
    assert weights == [1.0, 1.0, 1.0]
    a = _args('--views', 'orig;x1.5,hflip')
    assert (a.views_method, a.views_iou_thresh, a.views_soft_nms_cut, a.views_min_score) == ('weighted_fusion', 0.5, 1.0, 0)
    assert I.check_views(_args()) is None


def test_view_weights_are_normalised_by_their_maximum():
    assert I.check_views(_args('--views', 'orig;x1.5', '--views-weights', '2,1'))[2] == [1.0, 0.5]
    assert I.check_views(_args('--views', 'orig;x1.5', '--views-weights', '1,0.8'))[2] == [1.0, 0.8]
    for bad in ('1', '1,0.5,2', 'a,b', '0,0'):
        with pytest.raises(ValueError):
            I.check_views(_args('--views', 'orig;x1.5', '--views-weights', bad))


@pytest.mark.parametrize('spec', ['orig;x1.2,x1.5', 'orig;brute', 'orig;x1.5,bogus', 'orig;;x1.5', 'orig;dflip'])
def test_views_that_do_not_fold_into_the_preprocessing_kernel_are_rejected(spec):
    with pytest.raises(ValueError, match='--views'):
        I.check_views(_args('--views', spec))


@pytest.mark.parametrize('extra', [['--tta', 'x1.5'], ['-o', 'out'], ['--resume', 'd.pkl'], ['--eval', '--annotations', 'gt.json']])
def test_views_conflicting_flags_are_rejected(extra):
    with pytest.raises(ValueError, match='cannot be combined'):
        I.check_views(_args('--views', 'orig;x1.5', *extra))


def test_views_needs_export_and_one_process():
    a = I.build_parser().parse_args(['-i', 'imgs', '-o', 'out', '--views', 'orig;x1.5'])
    with pytest.raises(ValueError, match='needs --export'):
        I.check_views(a)
    with pytest.raises(NotImplementedError, match='-j N'):
        I.check_views(_args('--views', 'orig;x1.5', '-j', '2'))
    for extra in (['--export-views', 'v'], ['--views-weights', '1,1']):
        with pytest.raises(ValueError, match='need --views'):
            I.check_views(_args(*extra))
