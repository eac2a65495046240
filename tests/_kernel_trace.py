"""Which device kernels did a call launch?  A plain helper module for the GPU tests (not a conftest).

``launched(fn)`` runs ``fn`` under torch.profiler, synchronizes and returns the names of the device kernels that ran, in launch
order.  The ROCm profiler records this library's kernels with their template arguments
(``void (anonymous namespace)::conv_gather_kernel<4, 2, 2, 4, 32, false, 4, 1>(hc_conv_desc, int, int)``); the parsers below turn
those names into tuples so that a test can assert the exact instantiation the host dispatcher chose.  Older demanglers leave out
template arguments that equal their defaults (``conv_gather_kernel<2, 2, 2, 2, 64, false>``): both spellings parse to the same tuple.
"""
import re

import torch

# conv_gather_kernel<MR, NR, WM, WN, BK, FP8, NS = 2, MINB = 2> (csrc/conv_gather.hip)
_GATHER_DEFAULTS = (None, None, None, None, None, False, 2, 2)
_GATHER_RE = re.compile(r"\bconv_gather_kernel<([^<>]*)>")
# conv_pw_kernel<KS, STATS> (csrc/conv_pointwise.hip)
_PW_RE = re.compile(r"\bconv_pw_kernel<([^<>]*)>")


def _arg(text):
    text = text.strip()
    if text in ("true", "false"):
        return text == "true"
    return int(text.rstrip("uUlL"))


def _parse(pattern, name, defaults):
    m = pattern.search(name)
    if m is None:
        return None
    args = [_arg(a) for a in m.group(1).split(",")]
    if not args or len(args) > len(defaults):
        raise ValueError("unexpected template argument list in %r" % name)
    out = list(args) + list(defaults[len(args):])
    if any(v is None for v in out):
        raise ValueError("template arguments without a default missing in %r" % name)
    return tuple(out)


def parse_conv_gather(name):
    """``conv_gather_kernel<...>`` -> (MR, NR, WM, WN, BK, FP8, NS, MINB), or None for any other kernel."""
    return _parse(_GATHER_RE, name, _GATHER_DEFAULTS)


def parse_pw(name):
    """``conv_pw_kernel<KS, STATS>`` -> (KS, STATS), or None for any other kernel."""
    return _parse(_PW_RE, name, (None, None))


def launched(fn):
    """Run ``fn()`` under the profiler and return the names of the device kernels it launched.

    Raises AssertionError when the profiler recorded no device kernel at all: every caller passes a call that certainly launches
    one, so an empty list means the trace is broken, and a test that went on would assert nothing."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name for e in evs]
    if not names:
        raise AssertionError("torch.profiler recorded no device kernel for a call that launches one: the kernel trace is broken")
    return names


def gather_forms(names):
    """The conv_gather_kernel instantiations among ``names``, in launch order."""
    return [f for f in (parse_conv_gather(n) for n in names) if f is not None]


def pw_forms(names):
    return [f for f in (parse_pw(n) for n in names) if f is not None]


def launched_gather_form(fn):
    """Run ``fn()`` (exactly one gather-conv launch) and return its instantiation tuple."""
    names = launched(fn)
    forms = gather_forms(names)
    assert len(forms) == 1, ("expected one conv_gather_kernel launch", names)
    return forms[0]
