"""The reference's rank-1 and rank-3 SignalConv cases (python/layers/signal_conv_test.py:388-502, 620-735) and its
`is_implemented` rule with the rank condition (channel_separable needs rank <= 2), for channels-first arrays
[N, C, *support].  The SciPy oracle is the rank-generic one of signal_conv_cases.py.  Shared by the CPU tier (the
layers' pad / crop arithmetic around emulations of the kernels) and the GPU tier (the layers on the kernels)."""
import numpy as np

from signal_conv_cases import numpy_upsample, scipy_convolve_valid  # noqa: F401


def is_implemented(input_support, kernel_support, corr, strides_up, channel_separable, filters):
    """signal_conv_test.py:317-349."""
    odd = all(s % 2 == 1 for s in kernel_support)
    can_use_transpose = not corr or odd
    must_use_transpose = any(s != 1 for s in strides_up) or (not corr and not odd)
    if must_use_transpose and not can_use_transpose:
        return False
    if channel_separable and len(input_support) > 2:
        return False
    if channel_separable and any(s != strides_up[0] for s in strides_up):
        return False
    if channel_separable and must_use_transpose and filters != 1:
        return False
    return True


def _valid(support, channels, filters, ks, corr, sd, su, epe, sep, use_bias=False):
    return dict(input_support=support, channels=channels, filters=filters, kernel_support=ks, corr=corr,
                strides_down=sd, strides_up=su, extra_pad_end=epe, channel_separable=sep, use_bias=use_bias)


def valid_cases():
    """test_1d_valid_spatial, test_1d_valid_channels, test_1d_bias_activation and their rank-3 counterparts."""
    for sep in (False, True):
        for support in ((12,), (7,)):
            for ks in ((1,), (2,), (7,)):
                for corr in (False, True):
                    for sd, su, epe in zip([(1,), (1,), (1,), (1,), (1,), (2,), (5,), (2,)],
                                           [(1,), (2,), (2,), (3,), (3,), (1,), (1,), (3,)],
                                           [True, False, True, False, True, True, True, True]):
                        yield _valid(support, 1, 1, ks, corr, sd, su, epe, sep)
    for sep in (False, True):
        for channels, filters in zip([1, 2], [2, 1]):
            for su in ((1,), (2,)):
                yield _valid((9,), channels, filters, (3,), True, (1,), su, True, sep)
    yield _valid((6,), 1, 1, (3,), True, (1,), (1,), True, False, use_bias=True)
    for support in ((8, 7, 3), (5, 6, 4)):
        for ks in ((1, 2, 3), (2, 1, 2), (3, 3, 3)):
            for corr in (False, True):
                # (the reference zips 5 stride pairs against 4 extra_pad_end values: 4 cases)
                for sd, su, epe in zip([(1, 1, 1), (1, 1, 1), (1, 1, 1), (3, 5, 4), (2, 1, 1)],
                                       [(1, 1, 1), (1, 3, 2), (2, 4, 1), (1, 1, 1), (1, 1, 2)],
                                       [True, False, True, True]):
                    yield _valid(support, 1, 1, ks, corr, sd, su, epe, False)
    for channels, filters in zip([1, 2], [2, 1]):
        for su in ((1, 1, 1), (1, 2, 2)):
            yield _valid((7, 5, 4), channels, filters, (2, 3, 2), False, (1, 1, 1), su, False, False)
    yield _valid((7, 2, 4), 1, 1, (1, 2, 3), True, (1, 1, 1), (1, 1, 1), True, False, use_bias=True)
    # beyond the reference's lists: several channels with strides on both sides, and the rank-3 separable error
    yield _valid((11,), 5, 3, (5,), True, (2,), (1,), True, False, use_bias=True)
    yield _valid((5, 6, 7), 3, 4, (3, 3, 3), True, (1, 2, 2), (1, 1, 1), True, False, use_bias=True)
    yield _valid((4, 5, 6), 2, 3, (3, 3, 5), False, (2, 1, 1), (1, 2, 2), True, False)
    yield _valid((4, 5, 6), 1, 1, (3, 3, 3), True, (1, 1, 1), (1, 1, 1), True, True)


def same_cases():
    """test_1d_same_zeros_spatial, test_1d_same_padding and their rank-3 counterparts: identity kernels."""
    for support in ((12,), (7,)):
        for ks in ((1,), (2,), (3,), (7,)):
            for corr in (False, True):
                for sd, su, epe in zip([(1,), (1,), (1,), (2,), (5,), (2,)], [(1,), (2,), (3,), (1,), (1,), (3,)],
                                       [True, False, True, True, True, True]):
                    yield dict(input_support=support, kernel_support=ks, corr=corr, strides_down=sd, strides_up=su,
                               extra_pad_end=epe, padding="same_zeros")
    yield dict(input_support=(8,), kernel_support=(3,), corr=True, strides_down=(1,), strides_up=(1,),
               extra_pad_end=True, padding="same_reflect")
    for support in ((4, 5, 4), (5, 6, 3)):
        for ks in ((1, 2, 3), (2, 1, 2), (3, 3, 3)):
            for corr in (False, True):
                for sd, su, epe in zip([(1, 1, 1), (1, 1, 1), (1, 1, 1), (3, 5, 4)],
                                       [(1, 1, 1), (4, 3, 2), (2, 1, 3), (1, 1, 1)], [True, False, True, True]):
                    yield dict(input_support=support, kernel_support=ks, corr=corr, strides_down=sd, strides_up=su,
                               extra_pad_end=epe, padding="same_zeros")
    yield dict(input_support=(6, 6, 5), kernel_support=(3, 2, 2), corr=True, strides_down=(1, 1, 1),
               strides_up=(1, 1, 1), extra_pad_end=True, padding="same_reflect")


def identity_kernel(kernel_support):
    """initializers.IdentityInitializer for one channel and one filter: a unit impulse at support // 2."""
    k = np.zeros(tuple(kernel_support) + (1, 1), np.float32)
    k[tuple(s // 2 for s in kernel_support) + (0, 0)] = 1.0
    return k


def case_id(c):
    return "-".join(f"{k[:2]}{''.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in c.items())
