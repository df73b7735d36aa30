"""tests/gemm_epilogue_reference.py without a GPU: the model quotes DESIGN.md's contract, its inputs make every accumulator exact, its GELU is
torch's, every named defect misses the bars that tests/test_gpu_gemm_epilogues.py holds the kernels to on the very inputs that test uses, and the
kernel each of its cells names is the one the planner picks on 256 CUs."""
import ctypes

import pytest
import torch

import gemm_epilogue_reference as E
import row_reference as R

DTYPES = ("bf16", "fp32")
SMALL = [(dt,) + s for dt in DTYPES for s in E.small_input_sets(dt)]
LARGE = [("bf16", E.persistent_rows(256), 536, 64), ("fp32", E.persistent_rows(256), 536, 32), ("bf16",) + E.SPLIT_SHAPE]


def test_contract_is_the_text_of_design_md():
    assert E.CONTRACT == E.design_contract()


@pytest.mark.parametrize("dtype,M,N,K", SMALL + LARGE)
def test_inputs_make_the_accumulator_exact(dtype, M, N, K):
    """fp32 matmul == float64 matmul bit for bit (with and without the bias), a and w are bf16 numbers, every partial sum is inside the span
    in which multiples of 2^-12 are fp32 numbers, and the first bf16 rounding changes at least half of the elements."""
    inp = E.gemm_inputs(M, N, K)
    a, w, bias = inp["a"], inp["w"], inp["bias"]
    assert E.is_bf16(a) and E.is_bf16(w)
    for t, unit in ((a, 8), (w, 32), (bias, 4096)):
        assert torch.equal(t * unit, (t * unit).round())
    assert float(a.abs().max()) <= 1 and float(w.abs().max()) <= 0.125 and float(bias.abs().max()) < 1
    acc = E.accumulator(a, w, dtype)
    acc32 = a @ w.t()
    assert torch.equal(acc32.double(), acc)
    assert torch.equal((acc32 + bias).double(), acc + bias.double())
    assert E.exact_span(a, w, bias) < 2.0 ** 12
    share = E.first_rounding_share(acc, bias)
    std = float((acc + bias.double()).std())
    print(f"{dtype} {M}x{N}x{K}: pre-activation std {std:.2f}, first rounding changes {share:.1%}")
    assert share >= 0.5


def test_model_gelu_is_torchs():
    """The model's GELU and kept gelu' on a real input set against torch.nn.functional.gelu and autograd, in float64."""
    M, N, K = 300, 130, 72
    inp = E.gemm_inputs(M, N, K)
    form = E.form_named("fp32", "gelu_aux3_f32")
    bias, flags, aux, res, scale = E.form_call(form, inp, N)
    m = E.model(inp["a"], inp["w"], bias, flags, form.out, form.aux, aux, res, scale, dtype="fp32")
    v = (E.accumulator(inp["a"], inp["w"]) + bias.double()).requires_grad_(True)
    y = torch.nn.functional.gelu(v)
    y.sum().backward()
    assert float((m.g - y.detach()).abs().max()) < 1e-14
    assert float((m.kept_g - v.grad).abs().max()) < 1e-14
    assert torch.equal(m.c, E.f32(m.g)) and torch.equal(m.kept, E.f32(m.kept_g))


def _run(dtype, form, inp, acc, N, defect=None):
    """A form on the default geometry: the aux tensor of modes 2 / 4 is a view of its wider buffer, as on the device."""
    bias, flags, aux, res, scale = E.form_call(form, inp, N)
    geo = E.geometry(form, "vec", N)
    if aux is not None:
        c0, ld = geo["aux"]
        buf = torch.full((aux.shape[0] + 3, ld), -768.0)
        buf[1:1 + aux.shape[0], c0:c0 + N] = aux
        aux = buf[1:1 + aux.shape[0], c0:c0 + N]
    return E.model(inp["a"], inp["w"], bias, flags, form.out, form.aux, aux, res, scale, acc=acc, defect=defect, dtype=dtype,
                   ldc=geo["c"][1], ldaux=geo["aux"][1])


# the form in which a defect must show (bf16 inputs, fp32 inputs); `None`: the same name for both
CATCH = {"scale_after_round": ("scale_bf16_r", "scale_f32_r"), "no_pre_round_before_gelu": ("gelu_aux1_f32_r", None),
         "no_round_after_gelu": ("gelu_aux1_f32_r", None), "residual_before_gelu": ("gelu_res_f32_r", None),
         "bias_of_next_column": ("plain_bf16_r", "plain_f32"), "aux_row_stride_off": ("aux4_bf16_r", "aux4_f32"),
         "scale_cols_off_by_one": ("scale_bf16_r", "scale_f32"), "drop_last_k_tile": ("plain_f32", None),
         "gelu_grad_of_output": ("gelu_aux3_bf16_r", "gelu_aux3_f32")}
CATCH_KEPT = {"aux_row_stride_off": ("views_gelu_aux1_bf16_r", "views_gelu_aux1_f32"), "no_pre_round_before_gelu": ("gelu_aux1_f32_r", None)}


@pytest.mark.parametrize("dtype,M,N,K", SMALL)
def test_every_defect_misses_the_bars(dtype, M, N, K):
    """On every input set of the pinned and register-staged kernels: the model passes its own bars in every form, and what each defective model
    stores misses them in the form named for it (C, and the kept tensor where the defect is one of the kept tensor)."""
    assert set(CATCH) == set(E.DEFECTS)
    inp = E.gemm_inputs(M, N, K)
    acc = E.accumulator(inp["a"], inp["w"], dtype)
    clean = {f.name: _run(dtype, f, inp, acc, N) for f in E.forms(dtype)}
    for name, m in clean.items():
        assert max(E.excess(m, m.c, m.kept)) <= 1.0, name
    which = 0 if dtype == "bf16" else 1
    for defect in E.DEFECTS:
        seen = []
        for f in E.forms(dtype):
            bad = _run(dtype, f, inp, acc, N, defect)
            ec, ek = E.excess(clean[f.name], bad.c, bad.kept)
            if ec > 1.0:
                seen.append(f.name + ":C")
            if ek > 1.0:
                seen.append(f.name + ":aux")
        print(f"{dtype} {M}x{N}x{K} {defect}: {' '.join(seen)}")
        want = CATCH[defect][which] or CATCH[defect][0]
        assert want + ":C" in seen or want + ":aux" in seen, (defect, want, seen)
        if defect in CATCH_KEPT:
            want = CATCH_KEPT[defect][which] or CATCH_KEPT[defect][0]
            assert want + ":aux" in seen, (defect, want, seen)


def test_bars_reject_single_elements():
    """One element off by one ulp of its format fails a bit-equal form; one NaN fails every kind."""
    M, N, K = 37, 19, 10
    inp = E.gemm_inputs(M, N, K)
    acc = E.accumulator(inp["a"], inp["w"])
    for f in E.forms("bf16"):
        m = _run("bf16", f, inp, acc, N)
        got = m.c.clone()
        got[M - 1, N - 1] = float("nan")
        assert E.excess(m, got, m.kept)[0] > 1.0, f.name
        if m.c_kind == "exact":
            got = m.c.clone()
            got[M - 1, N - 1] += (R.bf16_ulp(got[M - 1, N - 1]) if f.out == "bf16" else E.ulp32(got[M - 1, N - 1]))
            assert E.excess(m, got, m.kept)[0] > 1.0, f.name


def _plan(q):
    from acai_omr_amd import _lib
    out, n = (_lib.AcaiGemmLaunch * 2)(), ctypes.c_int(-1)
    _lib.check(_lib.lib().acai_gemm_plan(ctypes.byref(q), out, ctypes.byref(n)), "acai_gemm_plan")
    return [out[i] for i in range(n.value)]


def _query(dtype, form, path, M, N, K, variant, lda=None, a_aligned=1, n_cu=256):
    from acai_omr_amd import _lib
    geo = E.geometry(form, path, N)
    esz = 2 if form.out == "bf16" else 4
    (c0, ldc), (x0, ldx), (r0, ldr) = geo["c"], geo["aux"], geo["res"]
    pc, px, pr = (ldc + c0) * esz, (ldx + x0) * esz, (ldr + r0) * 4      # byte offsets of the tensors (one row down) in 16-byte aligned buffers
    vec = E.expected_vec(form, N, pc, ldc, px, ldx, pr, ldr)
    q = _lib.AcaiGemmQuery(elem_size=2 if dtype == "bf16" else 4, epi=0, trans_a=0, trans_w=0, M=M, N=N, K=K, lda=lda or K, ldw=K, ldc=ldc,
                           ldr=ldr if form.res else 0, ldaux=ldx if form.aux else 0, a_aligned=a_aligned, w_aligned=1, c_aligned=int(pc % 16 == 0),
                           r_aligned=int(pr % 16 == 0) if form.res else 1, aux_aligned=int(px % 16 == 0) if form.aux else 1,
                           out_dtype=_lib.ACAI_BF16 if form.out == "bf16" else _lib.ACAI_F32,
                           flags=(E.GELU if form.gelu else 0) | (E.ROUND_BF16 if form.round else 0), aux_mode=form.aux, has_residual=int(form.res),
                           scale_cols=E.scale_cols(N) if form.scale else 0, want_colsum=0, variant=variant, n_cu=n_cu)
    return q, vec


@pytest.mark.parametrize("dtype", DTYPES)
def test_cells_name_the_planned_kernel(dtype):
    """Every cell of the GPU test, asked of the planner for 256 CUs: the kernel and the epilogue path the cell names are the ones planned, and each
    scalar-path cause switches the LDS-transposed epilogue off in the forms it concerns."""
    from acai_omr_amd import _lib
    kt = E.ktile(dtype)
    for kern in E.kernels_of(dtype):
        if kern in E.REG_KERNELS:
            M, N, K = (37, 19, 10) if kern == "reg_fast0_k10" else (300, 130, 72)
            lda, al = {"reg_fast0_lda": (K + 1, 1), "reg_fast0_off1": (K + 8, 0)}.get(kern, (K, 1))
            cells = [("vec", M, N, K, E.forms(dtype), lda, al)]
        else:
            cells = [(p, 1797, 262 if p == "n262" else 264, k, E.path_forms(dtype, p), None, 1) for p in E.PATHS for k in (kt, 3 * kt)]
            if kern in E.PERSISTENT:
                cells.append(("vec", E.persistent_rows(256), 536, kt, E.persistent_forms(dtype), None, 1))
        for path, M, N, K, fs, lda, al in cells:
            for f in fs:
                q, vec = _query(dtype, f, path, M, N, K, 0 if kern in E.REG_KERNELS else int(kern[1]), lda, al)
                plan = _plan(q)
                names = [_lib.GEMM_KERNEL_NAMES[l.kernel] + {_lib.GEMM_K_GLDS: f"<wm={l.wm}>", _lib.GEMM_K_REG: f"<fast={l.fast}>",
                                                             _lib.GEMM_K_PP: f"<mode={l.pp_mode}>"}.get(l.kernel, "") for l in plan]
                assert names == [E.expected_kernel(kern, f, vec)], (kern, path, f.name, names)
                assert plan[0].vec_epi == vec, (kern, path, f.name)
                if kern not in E.REG_KERNELS:
                    concerned = path in ("n262", "ldc", "c_off8") or (path == "ldr" and f.res) or (path == "ldaux" and f.aux)
                    assert vec == (0 if concerned else 1), (kern, path, f.name)


def test_split_shape_plans_two_launches():
    from acai_omr_amd import _lib
    M, N, K = E.SPLIT_SHAPE
    for name in E.SPLIT_FORMS:
        f = E.form_named("bf16", name)
        q, vec = _query("bf16", f, "vec", M, N, K, 0)
        plan = _plan(q)
        assert vec == 1 and [(l.kernel, l.row0, l.rows, l.vec_epi) for l in plan] == [(_lib.GEMM_K_PP, 0, 8192, 1), (_lib.GEMM_K_GLDS, 8192, 16, 1)], name
        assert plan[0].pp_mode == E.pp_mode(f) and plan[1].wm == 2
