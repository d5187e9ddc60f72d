// Test harness (CPU only): as parse_pipeline.cc, with everything a head stage at the audio carries.  One line per argument:
// `source|cmvn|utt2spk|norm_vars|kind:a:b,...|channel|min_duration|tolerance|F:<fields of eesen_fbank_opts_t>|P:<fields of
// eesen_pitch_opts_t>` (F: / P: empty without that extractor) or `NONE`.  tests/test_paste_cases.py compares it with
// eesen_amd/frontend.py.
#include <cstdio>
#include "../../eesen_amd/csrc/tools/feat_pipeline.h"
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    ktab::Pipeline p;
    if (!ktab::parse_feature_pipeline(argv[i], &p)) { std::printf("NONE\n"); continue; }
    std::printf("%s|%s|%s|%d|", p.source.c_str(), p.cmvn.c_str(), p.utt2spk.c_str(), p.norm_vars ? 1 : 0);
    for (size_t k = 0; k < p.stages.size(); ++k) std::printf("%s%d:%d:%d", k ? "," : "", p.stages[k].kind, p.stages[k].a, p.stages[k].b);
    std::printf("|%d|%.9g|%d|F:", p.has_fbank ? p.wave.channel : -1, p.has_fbank ? (double)p.wave.min_duration : 0.0, p.tolerance);
    if (p.has_fbank) {
      const eesen_fbank_opts_t& f = p.fbank;
      std::printf("%.9g,%.9g,%.9g,%.9g,%.9g,%d,%d,%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%d,%d,%.9g,%d,%d,%d,%.9g,%llu", f.samp_freq, f.frame_shift_ms,
                  f.frame_length_ms, f.dither, f.preemph_coeff, f.remove_dc_offset, f.window_type, f.round_to_power_of_two, f.snip_edges,
                  f.num_bins, f.low_freq, f.high_freq, f.vtln_low, f.vtln_high, f.htk_mode, f.use_energy, f.energy_floor, f.raw_energy,
                  f.htk_compat, f.use_log_fbank, f.vtln_warp, f.dither_seed);
    }
    std::printf("|P:");
    if (p.has_pitch) {
      const eesen_pitch_opts_t& q = p.pitch;
      std::printf("%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%d,%d,%d,%d,%d,%d,%d,%d,%.9g,%.9g,%.9g,%.9g,%.9g,%d,%d,%d,%d,%d,%d,%d,%d,%llu",
                  q.samp_freq, q.frame_shift_ms, q.frame_length_ms, q.preemph_coeff, q.min_f0, q.max_f0, q.soft_min_f0, q.penalty_factor,
                  q.lowpass_cutoff, q.resample_freq, q.delta_pitch, q.nccf_ballast, q.lowpass_filter_width, q.upsample_filter_width,
                  q.max_frames_latency, q.frames_per_chunk, q.simulate_first_pass_online, q.recompute_frame, q.nccf_ballast_online, q.snip_edges,
                  q.pitch_scale, q.pov_scale, q.pov_offset, q.delta_pitch_scale, q.delta_pitch_noise_stddev, q.normalization_left_context,
                  q.normalization_right_context, q.delta_window, q.delay, q.add_pov_feature, q.add_normalized_log_pitch, q.add_delta_pitch,
                  q.add_raw_log_pitch, q.noise_seed);
    }
    std::printf("\n");
  }
  return 0;
}
