"""No GPU: the build of the reference's own GPU kernels (oracle/_ref/libref_ops.so: oracle/Makefile, oracle/ref_shim/,
oracle/ref_glue.hip) and the conditions under which tests/test_reference_kernels_gpu.py compares them with the oracle and the HIP
ops (tests/reference_pin.py).  The library is never loaded here: it needs a GPU runtime."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import reference_pin as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_ops.so")
REFERENCE = os.environ.get("UNFLOW_REFERENCE", "/root/reference")
ENTRY_POINTS = ["ref_glue_correlation", "ref_glue_correlation_grad", "ref_glue_backward_warp", "ref_glue_backward_warp_grad",
                "ref_glue_forward_warp", "ref_glue_forward_warp_grad", "ref_glue_downsample"]


def test_reference_library_is_built_and_exports_the_seven_entry_points():
    assert os.path.exists(REF_SO), ("%s is missing: __graft_entry__.build() makes it where the reference checkout is present "
                                    "(make -C oracle _ref/libref_ops.so REFERENCE=<checkout>)" % REF_SO)
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", REF_SO], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()[-2:-1] == ["T"]}
    assert set(ENTRY_POINTS) <= exported, sorted(set(ENTRY_POINTS) - exported)
    # the reference's seven functions are in there too (C++ names), not stubs of ours
    for name in ("Correlation", "CorrelationGrad", "BackwardWarp", "BackwardWarpGrad", "ForwardWarp", "ForwardWarpGrad", "Downsample"):
        assert any(re.match(r"_Z%d%sRKN5Eigen9GpuDeviceE" % (len(name), name), s) for s in exported), name


def test_nothing_under_oracle_ref_is_tracked():
    r = subprocess.run(["git", "ls-files", "oracle/_ref"], cwd=ROOT, capture_output=True, text=True)
    if r.returncode == 0:
        assert r.stdout.strip() == ""
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()


def _line_set(path):
    """Normalised lines of three or more tokens (words and single punctuation marks, white space dropped)."""
    try:
        with open(path, encoding="utf-8") as f:
            text = f.read()
    except (UnicodeDecodeError, OSError):
        return set()
    lines = set()
    for line in text.splitlines():
        tokens = re.findall(r"\w+|[^\w\s]", line)
        if len(tokens) >= 3:
            lines.add(" ".join(tokens))
    return lines


def test_shim_and_glue_share_no_line_with_the_reference():
    """The stand-in headers and the glue are our own text: none of their lines of three or more tokens occurs in any file of
    the reference checkout (the normalised line-set check of VERDICT.md, "Copy-paste findings")."""
    if not os.path.isdir(os.path.join(REFERENCE, "ops")):
        pytest.skip("no reference checkout to compare with")
    ours = [os.path.join(ROOT, "oracle", "ref_glue.hip")]
    for d, _, files in os.walk(os.path.join(ROOT, "oracle", "ref_shim")):
        ours += [os.path.join(d, f) for f in files]
    assert len(ours) == 7, ours
    theirs = {}
    for d, _, files in os.walk(REFERENCE):
        if ".git" in d.split(os.sep):
            continue
        for f in files:
            p = os.path.join(d, f)
            if os.path.getsize(p) < (1 << 20):
                theirs[p] = _line_set(p)
    assert any(p.endswith("correlation_op.cu.cc") and s for p, s in theirs.items())
    shared = [(os.path.relpath(o, ROOT), os.path.relpath(p, REFERENCE), sorted(_line_set(o) & s)[:3])
              for o in ours for p, s in theirs.items() if _line_set(o) & s]
    assert not shared, shared


def test_makefile_and_build_hook_name_the_recipe():
    """The recipe compiles the reference's sources where they lie; no reference text is copied into the tree."""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    assert "_ref/libref_ops.so:" in mk and "$(REFERENCE)/ops/*_op.cu.cc" in mk and "--offload-arch=gfx950" in mk
    assert "-DGOOGLE_CUDA=1" in mk and "-Iref_shim" in mk and "-I$(REFERENCE)/ops" in mk
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "_ref/libref_ops.so" in f.read()


# ---------------------------------------------------------------- the conditions of the GPU comparison, with the oracle alone
def test_flows_are_dyadic_exact_in_fp32_and_cover_integers_zeros_and_outside():
    for size in R.WARP_SIZES:
        for C in R.WARP_CHANNELS:
            R.flow_conditions(R.warp_inputs(size, C)[1])


def test_gamma_is_a_bound_on_fp32_sums():
    """The bound of reference_pin on its own: 2000 products summed in fp32 forwards, backwards and pairwise stay within gamma of
    the fp64 sum, and a sum with one product dropped does not."""
    rs = np.random.RandomState(5)
    a, b = rs.randn(2000).astype(np.float32), rs.randn(2000).astype(np.float32)
    t = a.astype(np.float64) * b.astype(np.float64)
    v, S = t.sum() / 2000, np.abs(t).sum() / 2000
    g = R.gamma(2000, S)
    p32 = a * b
    fwd = np.float32(0)
    for x in p32:
        fwd = np.float32(fwd + x)
    bwd = np.float32(0)
    for x in p32[::-1]:
        bwd = np.float32(bwd + x)
    for s in (fwd, bwd, p32.sum(dtype=np.float32)):
        assert abs(np.float64(np.float32(s / np.float32(2000))) - v) <= g
    assert abs((t.sum() - t[np.argmax(np.abs(t))]) / 2000 - v) > g


@pytest.mark.parametrize("idx", range(len(R.CORR_CASES)), ids=R.CORR_IDS)
def test_oracle_correlation_within_gamma_of_fp64_every_element(idx, oracle_lib):
    """Share of elements that have to be excluded: zero."""
    in0, in1, dout = R.corr_inputs(idx)
    attrs = R.attrs_of(R.CORR_CASES[idx])
    ex = R.corr_exact(idx)
    out = oracle_lib.correlation(in0, in1, **attrs)
    assert out.shape == ex["out"][0].shape == dout.shape
    R.assert_within("oracle correlation %s" % R.CORR_IDS[idx], out, ex["out"])
    g0, g1 = oracle_lib.correlation_grad(dout, in0, in1, **attrs)
    R.assert_within("oracle correlation grad0 %s" % R.CORR_IDS[idx], g0, ex["grad0"])
    R.assert_within("oracle correlation grad1 %s" % R.CORR_IDS[idx], g1, ex["grad1"])


def test_oracle_one_hot_pair_lights_one_channel_at_one_site(oracle_lib):
    a, b = R.corr_one_hot_inputs()
    out = oracle_lib.correlation(a, b, **R.attrs_of(R.CORR_CASES[R.ONE_HOT_CASE]))
    assert len(np.argwhere(out != 0)) == 1
    v = R.corr_exact_fwd(a, b, *R.CORR_CASES[R.ONE_HOT_CASE][4:])[0]
    assert np.array_equal(np.argwhere(out != 0), np.argwhere(v != 0))


@pytest.mark.parametrize("size", R.WARP_SIZES, ids=str)
def test_oracle_warps_within_gamma_of_fp64_every_element(size, oracle_lib):
    for C in R.WARP_CHANNELS:
        im, flow, dout = R.warp_inputs(size, C)
        ex = R.warp_exact(size, C)
        tag = "%s C%d" % (size, C)
        R.assert_within("oracle backward_warp %s" % tag, oracle_lib.backward_warp(im, flow), ex["backward_warp"]["out"])
        R.assert_within("oracle backward_warp d_flow %s" % tag, oracle_lib.backward_warp_grad(dout, im, flow),
                        ex["backward_warp"]["d_flow"])
        assert np.any(ex["backward_warp"]["out"][2] < 4) and np.any(ex["backward_warp"]["out"][2] == 4)   # dropped taps occur
    im, flow, dout = R.warp_inputs(size, 1)
    ex = R.warp_exact(size, 1)["forward_warp"]
    R.assert_within("oracle forward_warp %s" % (size,), oracle_lib.forward_warp(flow), ex["out"])
    R.assert_within("oracle forward_warp d_flow %s" % (size,), oracle_lib.forward_warp_grad(dout, flow), ex["d_flow"])
    full = min(9, size[1]) * min(9, size[2])
    assert np.any(ex["d_flow"][2] == 0) and np.any(ex["d_flow"][2] == full)     # rejected sources and unclipped footprints occur


@pytest.mark.parametrize("scale", R.DOWNSAMPLE_SCALES)
def test_oracle_downsample_within_gamma_of_fp64_every_element(scale, oracle_lib):
    for shape in R.DOWNSAMPLE_SHAPES:
        im = R.ds_inputs(shape)
        R.assert_within("oracle downsample %s / %d" % (shape, scale), oracle_lib.downsample(im, scale), R.ds_exact(im, scale))
