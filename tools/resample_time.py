#!/usr/bin/env python3
"""Yardstick for f5e_resample (csrc/resample.hip) and for the voice-conversion pass built on it.

1. The op against the host route a caller had before (infer/audio.py::resample on the CPU, then the H2D copy of its result),
   for 10 s of mono audio at 24 k -> 16 k, 16 k -> 24 k, 44.1 k -> 24 k and 44.1 k -> 16 k.
   Kernel: 10 launches per graph (f5e_graph_*), HIP events around 5 replays.  Host route: wall clock, median of 5 synchronised
   passes after a warm one (the host convolution depends on the box's CPU and thread count: the count is recorded).
2. One utils_infer.infer_vc_process pass at the C5 utterance (configs/F5TTS_Small_PPG.yaml shape: dim 768, 18 blocks, seeded
   weights; prompt 188 frames = 2 s at 24 kHz, source 3 s at 44.1 kHz, NFE 32; default-size conformer PPG extractor, synthetic
   Vocos) against the same pass with every rate conversion done by the host route (device -> host, convolution, host ->
   device): wall clock from the call to the returned waveform, median of 5 after two warm passes.
Reports, not gates.  GPU box only:  python tools/resample_time.py [--out profiles/resample_time.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from f5e_tts_amd import ops  # noqa: E402
from f5e_tts_amd.infer import audio as A  # noqa: E402
from f5e_tts_amd.infer import utils_infer as U  # noqa: E402
from tools.mas_time import time_graph  # noqa: E402
from tools.src_hash import csrc_sha256  # noqa: E402

RATIOS = ((24000, 16000), (16000, 24000), (44100, 24000), (44100, 16000))
SECS, PASSES = 10, 5


def wall_median(fn, warm=1, reps=PASSES):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def host_route(w, orig_freq, new_freq):
    """What stood in for resample_device before: the audio on the host, the fp32 convolution there, the result uploaded."""
    return A.resample(w.cpu(), orig_freq, new_freq).to(w.device)


def vc_rig():
    from f5e_tts_amd.model import CFM, DiT
    from f5e_tts_amd.ppg import ConformerPPG, PPGModelWapper, kaldiFbank
    from f5e_tts_amd.vocoder import Vocos
    from tools import synth as SY
    arch = dict(dim=768, depth=18, heads=12, ff_mult=2, text_dim=512, conv_layers=4, text_num_embeds=2545,
                text_mask_padding=False, pe_attn_head=1)
    ppg_config = dict(use_ppg=True, ppg_dim=256, use_transformer=False)
    dit = DiT(**arch, ppg_config=ppg_config)
    dit.load_state_dict(SY.init_dit_state(SY.DiTConfig(**arch, use_ppg=True, ppg_dim=256), 1234), strict=True)
    cfm = CFM(transformer=dit, ppg_config=ppg_config).cuda().eval()
    torch.manual_seed(12)
    m = ConformerPPG(80, 218, global_cmvn=(torch.zeros(80), torch.ones(80)))
    for name, buf in m.named_buffers():          # BatchNorm statistics of a trained model are not (0, 1); keep them tame
        if name.endswith("running_var"):
            buf.fill_(1.1)
    front = object.__new__(PPGModelWapper)
    front.ppg_model, front.output_type, front.map_mix_ratio = m.cuda().eval(), "ppg", 1.0
    front.ppg_frame_length, front.mel_f_shift, front.device, front.stream = 20, 10, "cuda", False
    front.featCal = kaldiFbank().eval()
    voc = Vocos()
    voc.load_state_dict(SY.init_vocos_state(), strict=False)
    return cfm, front, voc.cuda().eval()


def main():
    ops.require_device()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [f"# python tools/resample_time.py on one MI355X; csrc_sha256 {csrc_sha256()}",
             f"# host: torch.get_num_threads() = {torch.get_num_threads()}; op: ms per launch, 10-launch graph, HIP events over 5 "
             f"replays; host route and passes: wall ms, median (min .. max) of {PASSES}"]
    side = torch.cuda.Stream()
    g = torch.Generator().manual_seed(1)
    for of, nf in RATIOS:
        orig, new, width, taps = A.resample_plan(of, nf)
        x = 0.1 * torch.randn(1, SECS * of, generator=g)
        xd = x.cuda()
        yd = torch.empty(1, -(-new * x.shape[1] // orig), device="cuda")
        op_ms = time_graph(lambda: ops.resample(xd, of, nf, out=yd), side)
        conv_ms = wall_median(lambda: A.resample(x, of, nf))
        route_ms = wall_median(lambda: A.resample(x, of, nf).cuda())
        back_ms = wall_median(lambda: host_route(xd, of, nf))
        err = float((yd.cpu() - A.resample(x, of, nf)).abs().max())
        lines.append(f"{of} -> {nf} ({orig}:{new}, {taps} taps, bank {new * taps * 4 / 1024:.1f} KiB), {SECS} s: f5e_resample "
                     f"{op_ms:8.4f} ms  |  host A.resample {conv_ms[0]:8.3f} ({conv_ms[1]:.3f} .. {conv_ms[2]:.3f}) ms; + H2D "
                     f"{route_ms[0]:8.3f} ({route_ms[1]:.3f} .. {route_ms[2]:.3f}) ms = {route_ms[0] / op_ms:7.1f} x the op; "
                     f"from device audio (D2H + conv + H2D) {back_ms[0]:8.3f} ms;  max |device - host| {err:.2e}")
        print(lines[-1], flush=True)

    cfm, front, voc = vc_rig()
    prompt = 0.05 * torch.randn(1, 188 * 256, generator=g)
    source = 0.05 * torch.randn(1, 3 * 44100, generator=g)
    kw = dict(nfe_step=32, alpha_spk=2.5, alpha_ppg=3.0, sway_sampling_coef=-1.0, seed=0, show_info=lambda m: None,
              device="cuda")

    def one_pass():
        return U.infer_vc_process((prompt, 24000), (source, 44100), cfm, voc, front, **kw)[0]

    dev_ms = wall_median(one_pass, warm=2)
    wave_dev = one_pass()
    device_route = A.resample_device
    A.resample_device = host_route
    try:
        host_ms = wall_median(one_pass, warm=2)
        wave_host = one_pass()
    finally:
        A.resample_device = device_route
    again_ms = wall_median(one_pass, warm=1)          # the device route once more, after the host legs (drift check)
    rel = float(abs(wave_dev - wave_host).max() / abs(wave_host).max())
    lines.append(f"infer_vc_process, C5 utterance (prompt 2 s at 24 kHz, source 3 s at 44.1 kHz, NFE 32): device resampling "
                 f"{dev_ms[0]:8.3f} ({dev_ms[1]:.3f} .. {dev_ms[2]:.3f}) ms, repeated after the host legs {again_ms[0]:8.3f} ms  |  "
                 f"host resampling {host_ms[0]:8.3f} ({host_ms[1]:.3f} .. {host_ms[2]:.3f}) ms;  "
                 f"difference {host_ms[0] - dev_ms[0]:+.3f} ms = {100 * (host_ms[0] - dev_ms[0]) / host_ms[0]:+.1f} % of the "
                 f"host-route pass;  waveforms differ by {rel:.2e} of the peak")
    print(lines[-1], flush=True)
    if out_path:
        with open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
