"""CPU: the kernel-name parsers of tests/_kernel_trace.py on the spellings the ROCm profiler records."""
import pytest

from _kernel_trace import gather_forms, parse_conv_gather, parse_pw, pw_forms


def test_parse_conv_gather_full_and_short_lists():
    full = "void (anonymous namespace)::conv_gather_kernel<4, 2, 2, 4, 32, false, 4, 1>(hc_conv_desc, int, int)"
    assert parse_conv_gather(full) == (4, 2, 2, 4, 32, False, 4, 1)
    # older demanglers leave out the arguments equal to the defaults (FP8 = false, NS = 2, MINB = 2)
    assert parse_conv_gather("conv_gather_kernel<2, 2, 2, 2, 64, false>") == (2, 2, 2, 2, 64, False, 2, 2)
    assert parse_conv_gather("void (anonymous namespace)::conv_gather_kernel<3, 1, 1, 4, 32, true>(hc_conv_desc, int, int)") == \
        (3, 1, 1, 4, 32, True, 2, 2)
    assert parse_conv_gather("conv_gather_kernel<1,2,1,4,32,false,2,4>") == (1, 2, 1, 4, 32, False, 2, 4)
    assert parse_conv_gather("void (anonymous namespace)::conv_pw_kernel<8, false>(...)") is None
    assert parse_conv_gather("Memcpy DtoD (Device -> Device)") is None
    with pytest.raises(ValueError):
        parse_conv_gather("conv_gather_kernel<2, 2, 2>")


def test_parse_pw_and_filters():
    names = ["void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >(int, ...)",
             "void (anonymous namespace)::conv_pw_kernel<4, true>(bf16_t const*, bf16_t const*, bf16_t*, float*, long, int, int, int, long, int)",
             "void (anonymous namespace)::conv_gather_kernel<1, 2, 2, 2, 64, false, 3, 2>(hc_conv_desc, int, int)"]
    assert parse_pw(names[1]) == (4, True)
    assert pw_forms(names) == [(4, True)]
    assert gather_forms(names) == [(1, 2, 2, 2, 64, False, 3, 2)]
