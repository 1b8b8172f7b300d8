"""Gaussian proposal augmentation without a GPU: the case table of tests/augment_ref.py really holds the conditions it names, the fp32
reference agrees with float64 statistics and draws what it says it draws, host.augmentation_normals is reproducible, and the binding,
host.Augment and the ops wrappers reject bad arguments before anything is launched."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import augment_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_the_listed_shapes_and_variants():
    cs = AR.cases()
    assert len({AR.case_id(c) for c in cs}) == len(cs)
    for form in ("tokens", "actions"):
        shapes = {c["shape"] for c in cs if c["form"] == form}
        assert shapes == set(AR.SHAPES) | (set(AR.FLOAT_ONLY) if form == "actions" else set())
        for s in shapes:                                            # every variant that can exist at a shape does
            got = {c["variant"] for c in cs if c["form"] == form and c["shape"] == s}
            assert got == {v for v in AR.VARIANTS if AR.feasible(form, s, v)}
            assert {"spread", "equal", "clip", "sigma0", "k0"} <= got
    assert {c["variant"] for c in cs if c["form"] == "tokens"} == set(AR.VARIANTS)
    assert {c["variant"] for c in cs if c["form"] == "actions"} == set(AR.VARIANTS) - {"midway", "outside"}


def _each(variant):
    cs = AR.cases(variants=(variant,))
    assert cs
    return [(c, AR.make_inputs(c), AR.case_reference(c)) for c in cs]


def test_variant_spread():
    some = 0
    for c, inp, r in _each("spread"):
        G, n, K, h = c["shape"]
        if n >= 2:
            assert (r["sd_raw"] > 0).all()
            some += 1
        assert np.isnan(inp["normals"][0, 0, 0, 0])                # the NaN normal lands on clip lo (the token of the first centre)
        assert r["v"][0, 0, 0, 0] == np.float32(-1.0)
        if c["form"] == "tokens":
            assert r["out"].reshape(G, n + K, h, 7)[0, n, 0, 0] == AR.TOK_VOCAB - 1
    assert some


def test_variant_equal_has_zero_sd():
    for c, inp, r in _each("equal"):
        assert (r["sd_raw"] == 0).all() and (r["sd"] == 0).all()
        G, n, K, h = c["shape"]
        out = r["out"].reshape(G, n + K, -1)
        assert (out == out[:, :1]).all()                           # mean = the sample, re-tokenised to its own centre


def test_variant_floor_is_active_on_some_dims_only():
    for c, inp, r in _each("floor"):
        active = r["sd_raw"] < np.float32(inp["sd_floor"])
        assert active.any() and not active.all()
        assert (r["sd"][active] == np.float32(inp["sd_floor"])).all() and (r["sd"][~active] == r["sd_raw"][~active]).all()


def test_variant_clip_is_active_on_some_values_only():
    for c, inp, r in _each("clip"):
        ok = ~np.isnan(r["unclipped"])
        clipped = (r["v"] != r["unclipped"]) & ok
        assert clipped.any() and not clipped[ok].all()
        assert r["v"].min() >= np.float32(inp["clip"][0]) and r["v"].max() <= np.float32(inp["clip"][1])


@pytest.mark.parametrize("first", (0, 1))
def test_variant_tie_goes_to_the_class_of_sample_0(first):
    for c, inp, r in _each(f"tie{first}"):
        G, n, K, h = c["shape"]
        assert (r["votes"][..., 0] == r["votes"][..., 1]).all() and (r["votes"].sum(-1) == n).all()
        x = AR.token_values(inp["tokens"], inp["centers"], AR.TOK_VOCAB).reshape(G, n, h, 7) if c["form"] == "tokens" \
            else inp["actions"].reshape(G, n, h, 7)
        assert ((x[:, 0, :, 6] >= 0.5) == bool(first)).all()
        assert (r["jwin"] == 0).all()
        out = r["out"].reshape(G, n + K, h, 7)
        assert (out[:, n:, :, 6] == out[:, :1, :, 6]).all()        # every augmented row carries sample 0's gripper


def test_variant_midway_has_two_nearest_centres():
    for c, inp, r in _each("midway"):
        d = np.abs((r["v"][..., None] - inp["centers"]).astype(np.float32))
        two = np.sort(d, axis=-1)[..., :2]
        assert (two[..., 0] == two[..., 1]).all() and (two[..., 0] == np.float32(1.0 / 256.0)).all()
        lower = np.argmax(d == two[..., :1], axis=-1)
        assert (r["bstar"] == lower).all()                         # first minimum wins: the lower index
        assert (np.abs(r["v"] - inp["centers"][r["bstar"] + 1]) == two[..., 0]).all()


def test_variant_sigma0_repeats_the_mean():
    for c, inp, r in _each("sigma0"):
        assert inp["sigma"] == 0.0
        assert (r["v"] == np.fmin(np.fmax(r["mean"], np.float32(-1)), np.float32(1))[:, None]).all()


def test_variant_k0_copies_the_originals_only():
    for c, inp, r in _each("k0"):
        assert inp["K"] == 0 and inp["normals"].shape[1] == 0
        src = inp["tokens"] if c["form"] == "tokens" else inp["actions"]
        assert r["out"].shape == src.shape and np.array_equal(r["out"], src)


def test_variant_outside_engages_the_clamp():
    for c, inp, r in _each("outside"):
        tok = inp["tokens"]
        b = AR.TOK_VOCAB - tok - 1
        assert (b < 0).any() and (b > AR.N_CENTERS - 1).any()
        x = AR.token_values(tok, inp["centers"], AR.TOK_VOCAB)
        assert (x[b < 0] == inp["centers"][0]).all() and (x[b > AR.N_CENTERS - 1] == inp["centers"][-1]).all()
        G, n, K, h = c["shape"]
        assert np.array_equal(r["out"].reshape(G, n + K, -1)[:, :n].reshape(G * n, -1), tok)    # copied verbatim, outside or not
        aug = r["out"].reshape(G, n + K, h, 7)[:, n:, :, :6]
        assert aug.min() >= AR.TOK_VOCAB - AR.N_CENTERS and aug.max() <= AR.TOK_VOCAB - 1


def test_originals_come_first_and_unchanged_in_every_case():
    for c in AR.cases():
        inp, r = AR.make_inputs(c), AR.case_reference(c)
        G, n, K, h = c["shape"]
        K = inp["K"]
        src = inp["tokens"] if c["form"] == "tokens" else inp["actions"]
        assert r["out"].dtype == src.dtype and r["out"].shape[0] == G * (n + K)
        assert np.array_equal(r["out"].reshape(G, n + K, -1)[:, :n].reshape(src.shape).view(np.int32 if src.dtype == np.float32 else np.int64),
                              src.view(np.int32 if src.dtype == np.float32 else np.int64))


# ------------------------------------------------------------------------------------------------ the reference against float64
def test_statistics_agree_with_float64():
    """mean to 1e-5 of the samples' magnitude (a mean that cancels to nearly zero cannot be held relative to itself), sd to 1e-5 relative."""
    n_checked = 0
    for c, inp, r in _each("spread"):
        G, n, K, h = c["shape"]
        if n < 2:
            continue
        x = (AR.token_values(inp["tokens"], inp["centers"], AR.TOK_VOCAB).reshape(G, n, h, 7) if c["form"] == "tokens"
             else inp["actions"].reshape(G, n, h, 7))[..., :6].astype(np.float64)
        mean64, sd64 = np.mean(x, axis=1), np.std(x, axis=1, ddof=1)
        scale = np.abs(x).max(axis=1)
        assert (np.abs(r["mean"] - mean64) <= 1e-5 * scale).all(), AR.case_id(c)
        assert (np.abs(r["sd"] - sd64) <= 1e-5 * sd64).all(), AR.case_id(c)
        n_checked += r["mean"].size
    assert n_checked > 1000


def test_augmented_rows_follow_the_fitted_gaussian():
    from cover_vla_amd import host
    G, n, K, h = 1, 5, 4096, 1
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.6, 0.6, (G * n, h, 7)).astype(np.float32)
    z = host.augmentation_normals(G, K, h, seed=11).numpy()
    for sigma in (1.0, 0.7):
        r = AR.reference_actions(x, n, K, z, sigma=sigma, sd_floor=0.0, clip=(-np.inf, np.inf))
        aug = r["out"].reshape(G, n + K, h, 7)[:, n:, :, :6].astype(np.float64)
        mean, sd = r["mean"].astype(np.float64), r["sd"].astype(np.float64)
        m_hat, s_hat = aug.mean(axis=1), aug.std(axis=1, ddof=1)
        assert (np.abs(m_hat - mean) <= 5.0 * sigma * sd / np.sqrt(K)).all()
        assert (np.abs(s_hat - sigma * sd) <= 0.10 * sigma * sd).all()


# ------------------------------------------------------------------------------------------------ host
def test_augmentation_normals_are_reproducible_per_seed():
    from cover_vla_amd import host
    a, b, c = host.augmentation_normals(3, 60, 2, seed=7), host.augmentation_normals(3, 60, 2, seed=7), host.augmentation_normals(3, 60, 2, seed=8)
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 60, 2, 6) and a.device.type == "cpu" and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert tuple(host.augmentation_normals(2, 0, 1, seed=0).shape) == (2, 0, 1, 6)
    assert abs(float(a.mean())) < 0.2 and 0.8 < float(a.std()) < 1.2
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            host.augmentation_normals(*bad, seed=0)


def test_host_augment_checks_its_values():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    z = host.augmentation_normals(2, 5, 4, seed=1)
    a = host.Augment(3, 5, z)
    assert a.samples_per_prompt == 3 and a.n_augmented == 5 and a.normals is z and a.sigma == 1.0 and a.sd_floor == 0.0 and a.clip == (-1.0, 1.0)
    assert host.Augment(3, 5, z, sigma=0.5, sd_floor=0.01, clip=(-np.inf, np.inf)).clip == (-np.inf, np.inf)
    assert tuple(a) == (3, 5, z, 1.0, 0.0, (-1.0, 1.0))
    bad = [dict(samples_per_prompt=0), dict(samples_per_prompt=4097), dict(samples_per_prompt=2.0), dict(n_augmented=-1), dict(n_augmented=4097),
           dict(n_augmented=4), dict(normals=z.double()), dict(normals=z.numpy()), dict(normals=z[..., :5]), dict(normals=z[0]),
           dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma="1"), dict(sd_floor=-0.1), dict(sd_floor=float("nan")),
           dict(clip=(1.0, -1.0)), dict(clip=(0.0,)), dict(clip=1.0), dict(clip=(float("nan"), 1.0))]
    for over in bad:
        kw = dict(samples_per_prompt=3, n_augmented=5, normals=z)
        kw.update(over)
        with pytest.raises(CoverError):
            host.Augment(**kw)


def test_wrappers_validate_without_a_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    G, n, K, h = 2, 3, 4, 2
    tok = torch.full((G * n, 7 * h), AR.TOK_VOCAB - 100, dtype=torch.int64)
    act = torch.zeros(G * n, h, 7)
    z = torch.zeros(G, K, h, 6)
    cen = torch.from_numpy(AR.openvla_centers())
    T = lambda **kw: ops.augment_tokens(kw.pop("tokens", tok), kw.pop("n", n), kw.pop("K", K), kw.pop("normals", z), kw.pop("centers", cen),
                                        AR.TOK_VOCAB, **{"steps": h, **kw})
    A = lambda **kw: ops.augment_actions(kw.pop("actions", act), kw.pop("n", n), kw.pop("K", K), kw.pop("normals", z), **kw)
    common = [dict(n=0), dict(n=4), dict(n=4097), dict(K=-1), dict(K=4097), dict(K=5),
              dict(normals=z.double()), dict(normals=z.numpy()), dict(normals=z[:, :, :1]), dict(normals=torch.zeros(G, K, h, 12)[..., ::2]),
              dict(normals=z.reshape(G * K, h, 6)), dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e39),
              dict(sd_floor=-1e-3), dict(sd_floor=float("nan")), dict(sd_floor=float("inf")), dict(clip=(0.5, -0.5)), dict(clip=(float("nan"), 1.0)),
              dict(clip=0.5), dict(clip=(1.0,))]
    for kw in common:
        with pytest.raises(CoverError):
            T(**dict(kw))
        with pytest.raises(CoverError):
            A(**dict(kw))
    for kw in (dict(tokens=tok.int()), dict(tokens=tok.numpy()), dict(tokens=tok[0]), dict(tokens=tok[:, :13]), dict(tokens=tok.t().contiguous().t()),
               dict(steps=0), dict(steps=3), dict(centers=cen.double()), dict(centers=cen[None]), dict(centers=cen[:0]), dict(centers=cen.numpy()),
               dict(out=torch.zeros(G * (n + K), 7 * h)), dict(out=torch.zeros(G * n, 7 * h, dtype=torch.int64)),
               dict(tokens=torch.zeros(65 * 7, dtype=torch.int64).expand(G * n, 65 * 7), steps=65, normals=torch.zeros(G, K, 65, 6))):
        with pytest.raises(CoverError):
            T(**kw)
    for kw in (dict(actions=act.double()), dict(actions=act.numpy()), dict(actions=act[0]), dict(actions=act[..., :6]),
               dict(actions=torch.zeros(G * n, h, 14)[..., ::2]), dict(out=torch.zeros(G * (n + K), h, 7, dtype=torch.float64)),
               dict(out=torch.zeros(G * (n + K), h, 8)[..., :7]), dict(actions=torch.zeros(G * n, 65, 7), normals=torch.zeros(G, K, 65, 6))):
        with pytest.raises(CoverError):
            A(**kw)
    # valid arguments on host tensors: there is no CPU path
    for call in (T, A):
        with pytest.raises(CoverError, match="device"):
            call()
        with pytest.raises(CoverError, match="device"):
            call(K=0, normals=torch.zeros(G, 0, h, 6), stats=True, clip=(-float("inf"), float("inf")))
    with pytest.raises(CoverError, match="device"):
        ops.augment_actions(torch.zeros(G * n, h + 1, 32)[:, :h, :7], n, K, z)        # the strided view is accepted as it is


def test_signatures_default_to_off():
    from cover_vla_amd import host, ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0 import PI0Policy
    p = inspect.signature(ops.augment_tokens).parameters
    assert list(p)[:6] == ["tokens", "n_samples", "n_augmented", "normals", "centers", "tok_vocab"]
    assert [(k, p[k].default) for k in list(p)[6:]] == [("steps", 1), ("sigma", 1.0), ("sd_floor", 0.0), ("clip", (-1.0, 1.0)), ("out", None),
                                                         ("stats", False)]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    p = inspect.signature(ops.augment_actions).parameters
    assert list(p)[:4] == ["actions", "n_samples", "n_augmented", "normals"] and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    assert ops.AugmentStats._fields == ("mean", "sd", "votes")
    p = inspect.signature(PI0Policy.select_action).parameters
    assert list(p) == ["self", "batch", "noise", "noise_std", "augment"] and p["augment"].default is None
    p = inspect.signature(OpenVLA.augment).parameters
    assert list(p) == ["self", "tokens", "n_samples", "n_augmented", "normals", "sigma", "sd_floor"]
    assert p["sigma"].default == 1.0 and p["sd_floor"].default == 0.0
    assert host.Augment._fields == ("samples_per_prompt", "n_augmented", "normals", "sigma", "sd_floor", "clip")
    assert "tie" in ops.augment_tokens.__doc__.lower() and "NaN" in ops.augment_tokens.__doc__ and "tie" in host.Augment.__doc__


# ------------------------------------------------------------------------------------------------ binding
_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cover_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(cover_augment_args, f));
int main(void) {
    printf("sizeof %zu\n", sizeof(cover_augment_args));
    F(src) F(n_stride) F(t_stride) F(normals) F(centers) F(n_centers) F(tok_vocab) F(G) F(n) F(K) F(h) F(sigma) F(sd_floor) F(clip_lo)
    F(clip_hi) F(out) F(mean_out) F(sd_out) F(votes_out)
    return 0;
}
"""


def test_struct_mirror_matches_a_compiled_probe_of_the_header(tmp_path):
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_augment_args"] is L.AugmentArgs
    for sym in ("cover_augment_tokens", "cover_augment_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.AugmentArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_augment_tokens(const cover_augment_args* args, void* stream);" in hdr
    assert "int cover_augment_actions(const cover_augment_args* args, void* stream);" in hdr
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed to probe include/cover_hip.h"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(L.AugmentArgs) == 112
    assert list(out) == [f[0] for f in L.AugmentArgs._fields_]
    for name, _ in L.AugmentArgs._fields_:
        assert int(out[name]) == getattr(L.AugmentArgs, name).offset, name
    if os.path.exists(L.LIB_PATH):                                   # cover_sizeof is host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_augment_tokens") and hasattr(h, "cover_augment_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_augment_args") == C.sizeof(L.AugmentArgs)
