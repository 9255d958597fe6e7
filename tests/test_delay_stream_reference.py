"""Streaming blind delay mask without a GPU: the C ABI's surface (struct layout, exports, the
host-side error table through avz_delay_stream_check) and the properties of the fp64
restatement avz.delay_mask.delay_mask_stream_numpy / NumpyDelayStream that the GPU tests
compare the kernel with: grouping, the relation to the offline histogram, the adapt gate,
power-of-two scaling, the stability caps of the shared cases, and the mutations the GPU test's
criteria must catch (figures in DESIGN.md section 19)."""
import ctypes as ct
import os
import subprocess

import numpy as np

from conftest import ROOT

import delay_mask_cases as DC
import delay_stream_cases as SC
from avz import _lib
from avz import delay_mask as DM


def _cfg(**kw):
    c = _lib.AvzConfig(fs=16000, n_fft=1024, hop=512, sigma=1e-5, angle_deg=90.0, mic_d=0.08,
                       c_sound=343.0, fmin_hz=100.0, mask_mode=_lib.MASK_EXTERNAL,
                       postfilter=_lib.PF_EXT_FLOOR, pf_floor=0.05, weight_eps=0.0,
                       normalize=_lib.NORM_NONE, norm_eps=0.0, max_batch=4, max_samples=64000)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


F1024, HOPS = 513, 6
STATE_1024_65 = 4864  # 64 + 2 * 512 * 4 + 65 * 8 = 4680, rounded up to 256


def _args(**kw):
    p = 4096  # any non-null, 256-byte aligned address: the checks never dereference
    a = _lib.AvzDelayStreamArgs(streams=2, hops=HOPS, forget=1.0, mix=p, mix_stride=2 * HOPS * 512,
                                ch_stride=HOPS * 512, hist_bins=65, smooth=3, max_peaks=3,
                                rel_height=0.25, min_sep=0.2, f_lo_hz=100.0, mask=p,
                                mask_stride_b=F1024 * HOPS, mask_stride_f=HOPS, mask_stride_t=1,
                                state=p, state_bytes=2 * STATE_1024_65)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_exports_version_and_struct_layout(tmp_path):
    lib = _lib.lib
    for n in ("avz_delay_stream_state_bytes", "avz_delay_stream_reset", "avz_delay_stream_push",
              "avz_delay_stream_check"):
        assert n in _lib.EXPORTED and hasattr(lib, n)
    assert lib.avz_version() == _lib.ABI_VERSION
    hdr = os.path.join(ROOT, "include", "avz.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(avz_delay_stream_args));']
    for f, _ in _lib.AvzDelayStreamArgs._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(avz_delay_stream_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                  check=True).stdout.splitlines())
    assert int(got["size"]) == ct.sizeof(_lib.AvzDelayStreamArgs)
    for f, _ in _lib.AvzDelayStreamArgs._fields_:
        assert int(got[f]) == getattr(_lib.AvzDelayStreamArgs, f).offset, f


def test_host_side_checks_reject_before_any_device_work():
    lib, E = _lib.lib, _lib
    chk = lambda c=None, **kw: lib.avz_delay_stream_check(ct.byref(c or _cfg()), ct.byref(_args(**kw)))  # noqa
    assert chk() == E.AVZ_OK
    # the public entry points without a plan; NULL configuration or arguments
    assert lib.avz_delay_stream_push(None, ct.byref(_args()), None) == E.AVZ_ERR_ARG
    assert lib.avz_delay_stream_reset(None, 4096, 1 << 20, 2, 65, None, None) == E.AVZ_ERR_ARG
    assert lib.avz_delay_stream_state_bytes(None, 1, 65) == E.AVZ_ERR_ARG
    assert lib.avz_delay_stream_check(None, ct.byref(_args())) == E.AVZ_ERR_ARG
    assert lib.avz_delay_stream_check(ct.byref(_cfg()), None) == E.AVZ_ERR_ARG
    # AVZ_ERR_ARG: NULL pointers (the optional ones may be NULL), parameters outside their range
    for name in ("mix", "mask", "state"):
        assert chk(**{name: None}) == E.AVZ_ERR_ARG, name
    assert chk(active=None, adapt=None, angle_deg=None, hist_out=None, delays_out=None,
               n_peaks=None) == E.AVZ_OK
    assert chk(active=4096, adapt=4096, angle_deg=4096, hist_out=4096, delays_out=4096,
               n_peaks=4096) == E.AVZ_OK
    for h in (0, -1):
        assert chk(hops=h) == E.AVZ_ERR_ARG, h
    for f in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert chk(forget=f) == E.AVZ_ERR_ARG, f
    assert chk(forget=1e-3) == E.AVZ_OK
    for nb in (7, 8, 64, 66, 259, 0, -65):
        assert chk(hist_bins=nb) == E.AVZ_ERR_ARG, nb
    for nb in (9, 65):
        assert chk(hist_bins=nb) == E.AVZ_OK, nb
    assert chk(hist_bins=257, state_bytes=1 << 20) == E.AVZ_OK
    for s in (-1, 9):
        assert chk(smooth=s) == E.AVZ_ERR_ARG, s
    for s in (0, 8):
        assert chk(smooth=s) == E.AVZ_OK, s
    for m in (-1, 8):
        assert chk(max_peaks=m) == E.AVZ_ERR_ARG, m
    for m in (0, 7):
        assert chk(max_peaks=m) == E.AVZ_OK, m
    for r in (0.0, -0.25, 1.0000001, float("nan"), float("inf")):
        assert chk(rel_height=r) == E.AVZ_ERR_ARG, r
    assert chk(rel_height=1.0) == E.AVZ_OK
    for name in ("min_sep", "f_lo_hz"):
        for v in (-1e-9, float("nan")):
            assert chk(**{name: v}) == E.AVZ_ERR_ARG, (name, v)
        assert chk(**{name: 0.0}) == E.AVZ_OK, name
    # AVZ_ERR_SHAPE: streams, strides shorter than a row, overlapping mask elements, the state
    for b in (0, -1, 5):
        assert chk(streams=b) == E.AVZ_ERR_SHAPE, b
    assert chk(streams=4, state_bytes=4 * STATE_1024_65) == E.AVZ_OK
    assert chk(ch_stride=HOPS * 512 - 1) == E.AVZ_ERR_SHAPE
    assert chk(mix_stride=2 * HOPS * 512 - 1) == E.AVZ_ERR_SHAPE
    assert chk(streams=1, mix_stride=0, mask_stride_b=0) == E.AVZ_OK   # one row: no row stride
    assert chk(mask_stride_f=HOPS - 1) == E.AVZ_ERR_SHAPE               # bins overlap
    assert chk(mask_stride_b=F1024 * HOPS - 1) == E.AVZ_ERR_SHAPE       # rows overlap
    assert chk(mask_stride_t=0) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=0) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=-HOPS) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=1, mask_stride_t=F1024) == E.AVZ_OK        # [streams, hops, F]
    assert chk(mask_stride_f=1, mask_stride_t=F1024 - 1) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=1, mask_stride_t=F1024, mask_stride_b=F1024 * HOPS - 1) \
        == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=2 * HOPS, mask_stride_t=2, mask_stride_b=2 * F1024 * HOPS) == E.AVZ_OK
    assert chk(hops=1, ch_stride=512, mix_stride=1024, mask_stride_f=1, mask_stride_t=1,
               mask_stride_b=F1024) == E.AVZ_OK                         # one hop: [streams, F, 1]
    assert chk(state_bytes=2 * STATE_1024_65 - 1) == E.AVZ_ERR_SHAPE
    assert chk(state_bytes=0) == E.AVZ_ERR_SHAPE
    assert chk(hist_bins=257) == E.AVZ_ERR_SHAPE       # 64 + 4096 + 2056 -> 6400 B per stream
    assert chk(hist_bins=257, state_bytes=2 * 6400) == E.AVZ_OK
    assert chk(hist_bins=257, state_bytes=2 * 6400 - 1) == E.AVZ_ERR_SHAPE
    # AVZ_ERR_ALIGN: the state's 256 bytes
    for off in (1, 8, 128):
        assert chk(state=4096 + off) == E.AVZ_ERR_ALIGN, off
    # the plan's mask mode, beamformer, post-filter and normalisation are ignored
    assert chk(_cfg(mask_mode=E.MASK_IBM, postfilter=E.PF_IBM_TARGET)) == E.AVZ_OK
    assert chk(_cfg(beamformer=E.BF_HYBRID_NULL, mask_mode=E.MASK_IPD, postfilter=E.PF_NONE,
                    normalize=E.NORM_PEAK)) == E.AVZ_OK
    small = _cfg(n_fft=512, hop=256)
    assert chk(small, ch_stride=HOPS * 256, mix_stride=2 * HOPS * 256,
               state_bytes=2 * 2816) == E.AVZ_OK                        # 64 + 2048 + 520 -> 2816
    assert chk(small, ch_stride=HOPS * 256, mix_stride=2 * HOPS * 256,
               state_bytes=2 * 2816 - 1) == E.AVZ_ERR_SHAPE


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_grouping_does_not_change_the_restatement():
    for N, d in SC.CASES:
        H = N // 2
        x = SC.inputs(N, d)[1]
        Y = SC.spectra(N, d, 1)
        for forget in SC.FORGETS:
            kw = dict(fs=SC.FS, mic_d=d, c_sound=SC.C_SOUND, forget=forget)
            whole = DM.NumpyDelayStream(N, **kw).push(x)
            spec = DM.delay_mask_stream_numpy(Y[0], Y[1], N, SC.FS, d, SC.C_SOUND, forget=forget)
            for name, groups in SC.GROUPINGS.items():
                a, b = DM.NumpyDelayStream(N, **kw), DM.NumpyDelayStream(N, **kw)
                pa, pb, j = [], [], 0
                for g in groups:
                    pa.append(a.push(x[:, j * H:(j + g) * H]))
                    pb.append(b.push_spectra(Y[0][:, j:j + g], Y[1][:, j:j + g]))
                    j += g
                cat = lambda ps: [np.concatenate([p[i] for p in ps], axis=1 if i == 0 else 0)  # noqa
                                  for i in range(4)]
                assert _same(cat(pa), whole), (N, d, forget, name)
                assert _same(cat(pb), spec), (N, d, forget, name)
                assert a.count == b.count == SC.T
            # the frames push() forms are the library's STFT frames up to its fp32 rounding
            top = spec[1][-1].max()
            assert np.abs(whole[1][-1] - spec[1][-1]).max() <= 1e-3 * top


def test_forget_one_ends_at_the_offline_histogram():
    for N, d in SC.CASES:
        for s in range(SC.STREAMS):
            r = SC.reference(N, d, s, 1.0)
            h = DM.delay_histogram(r["Y"][0], r["Y"][1], r["grid"])
            err = np.abs(r["h"][-1] - h).max() / h.max()
            print(f"N={N} d={d} [{s}]: |h_T - h_offline| = {err:.1e} of max h")
            assert err <= 1e-12
            # and the labels of the last frame are the offline mask's when the lists agree
            delays, J, bins = DM.delay_peaks(h, r["grid"])
            assert bins == r["bins"][-1]
            off = DM.delay_labels(r["Y"][0], r["Y"][1], delays, J, N)
            assert np.array_equal(off[:, -1], r["M"][:, -1])


def test_adapt_gate_freezes_the_histogram_while_labels_continue():
    adapt = np.ones(SC.T, int)
    adapt[5:9] = 0
    for N, d in SC.CASES:
        for forget in SC.FORGETS:
            base = SC.reference(N, d, 0, forget)
            r = SC.run_numpy(base["Y"], N, d, forget, adapt=adapt)
            assert np.array_equal(r["h"][:5], base["h"][:5])
            for t in range(5, 9):
                assert np.array_equal(r["h"][t], r["h"][4])
                assert np.array_equal(r["lists"][t], r["lists"][4], equal_nan=True)
            assert not np.array_equal(r["h"][9], r["h"][8])
            # frozen lists, live labels: frames 5 .. 8 are labelled with frame 4's list
            want = SC.labels_at(base["Y"][:, :, 5:9], [r["lists"][4]] * 4, [r["J"][4]] * 4, N)
            assert np.array_equal(r["M"][:, 5:9], want)
            assert len({r["M"][:, t].tobytes() for t in range(5, 9)}) > 1


def test_power_of_two_scaling_changes_no_list_and_no_label():
    for N, d in SC.CASES:
        for forget in SC.FORGETS:
            for s in range(SC.STREAMS):
                r = SC.reference(N, d, s, forget)
                for e in (10, -10):
                    Y = (r["Y"] * np.float32(2.0 ** e)).astype(np.complex64)
                    q = SC.run_numpy(Y, N, d, forget)
                    assert np.array_equal(q["J"], r["J"])
                    assert np.array_equal(q["lists"], r["lists"], equal_nan=True)
                    assert np.array_equal(q["M"], r["M"])
                    assert np.array_equal(q["h"], r["h"] * 4.0 ** e)


def test_caps_hold_on_the_restatement_alone():
    """At most 2 unstable frames and at most 1 % unstable decisions per stream."""
    for N, d in SC.CASES:
        for forget in SC.FORGETS:
            for s in range(SC.STREAMS):
                r = SC.reference(N, d, s, forget)
                M, stable = SC.stable_labels(r, r["lists"], r["J"])
                assert np.array_equal(M, r["M"])
                bad = np.flatnonzero(~r["stable"])
                top = r["h"].max(axis=1)
                print(f"N={N} d={d} forget={forget} [{s}]: unstable frames {bad.tolist()}, "
                      f"unstable decisions {100 * (1 - stable.mean()):.3f} %, E_pert "
                      f"{(r['e_pert'] / top).min():.1e} - {(r['e_pert'] / top).max():.1e} of max "
                      f"h_t, D_pert <= {r['d_pert'].max():.1e}, J {r['J'].min()} - {r['J'].max()}")
                assert len(bad) <= 2
                assert 1 - stable.mean() <= 0.01
                assert (top > 0).all() and (r["M"][0] == 1.0).all()


def _mutant(Y, N, d, forget, kind, adapt=None):
    """The restatement with one defect: 'lag' labels frame t with frame t - 1's list (none for
    t = 0), 'post' applies forget to h_t-1 + d_t, 'noforget' ignores forget, 'noadapt' ignores
    the adapt flags."""
    g = DM.delay_grid(N, SC.FS, d, SC.C_SOUND)
    Tn = Y.shape[2]
    h = np.zeros(g.nb)
    hs, M = np.empty((Tn, g.nb)), np.empty((Y.shape[1], Tn), np.float32)
    prev = (DM.delay_peaks(h, g)[0], 0)
    for t in range(Tn):
        y0, y1 = Y[0][:, t:t + 1], Y[1][:, t:t + 1]
        dt = DM.delay_histogram(y0, y1, g)
        if adapt is None or adapt[t] or kind == "noadapt":
            h = {"post": forget * (h + dt), "noforget": h + dt}.get(kind, forget * h + dt)
        delays, J, _ = DM.delay_peaks(h, g)
        use = prev if kind == "lag" else (delays, J)
        M[:, t] = DM.delay_labels(y0, y1, use[0], use[1], N)[:, 0]
        prev, hs[t] = (delays, J), h
    return M, hs


def test_mutations_exceed_the_gpu_criteria():
    """Each defect, evaluated on the restatement, fails the GPU test's criterion on every case
    and stream: labels on stable decisions, or hist_out's 4 E_pert(t) + 2^-20 max h_t."""
    adapt = np.ones(SC.T, int)
    adapt[5:9] = 0
    for N, d in SC.CASES:
        for s in range(SC.STREAMS):
            r = SC.reference(N, d, s, 0.9)
            top, tol = r["h"][-1].max(), SC.hist_tolerance(r, SC.T - 1)
            _, stable = SC.stable_labels(r, r["lists"], r["J"])
            M, hs = _mutant(r["Y"], N, d, 0.9, "lag")
            assert np.array_equal(hs, r["h"])
            diff = M != r["M"]
            msg = f"N={N} d={d} [{s}]: lagging list {100 * diff.mean():.1f} % of labels"
            assert (diff & stable).sum() > 0
            for kind in ("post", "noforget"):
                _, hs = _mutant(r["Y"], N, d, 0.9, kind)
                err = np.abs(hs[-1] - r["h"][-1]).max()
                msg += f", {kind} {100 * err / top:.0f} % of max h"
                assert err > tol, (kind, err, tol)
            for forget in SC.FORGETS:
                g = SC.reference(N, d, s, forget, adapt=adapt, key="gate")
                _, hs = _mutant(g["Y"], N, d, forget, "noadapt", adapt)
                err = np.abs(hs[-1] - g["h"][-1]).max()
                msg += f", gate ignored (forget {forget}) {100 * err / g['h'][-1].max():.0f} %"
                assert err > SC.hist_tolerance(g, SC.T - 1), (forget, err)
            print(msg + f" (tolerance {100 * tol / top:.2f} %)")


def test_end_to_end_restatement_chain_and_its_spread():
    """The 4-s scene through delay_mask_stream_numpy -> stream_numpy: its SIR, the MPDR
    baseline and the spread over the 8 perturbations whose 4-fold is the GPU test's margin."""
    e = SC.e2e_reference()
    print(f"restatement chain: SIR {e['sir']:.2f} dB, all-zero mask {e['sir_mpdr']:.2f} dB, "
          f"spread over the perturbations {e['spread']:.3f} dB")
    assert e["sir"] >= e["sir_mpdr"] + 10.0
    assert e["spread"] < 0.5 * (e["sir"] - e["sir_mpdr"])
