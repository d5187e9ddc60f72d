// class_prior.h -- the log-priors of net-output-extract's --class-frame-counts (shared by net_output_extract.cc and ctc_align.cc).
#pragma once
#include <cfloat>
#include <cmath>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

// ClassPrior::ClassPrior (class-prior.cc:30-77): counts -> floor -> blank scaling -> normalise -> log, with FLT_MAX/2 added
// for the classes below the cutoff so that they get zero likelihood
inline std::vector<float> class_log_priors(const std::string& path, double prior_cutoff, double blank_scale) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::string txt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  for (char& c : txt) if (c == '[' || c == ']') c = ' ';
  std::istringstream ss(txt);
  std::vector<double> pri;
  for (double v; ss >> v;) pri.push_back(v);
  std::vector<float> mask(pri.size(), 0.f);
  for (size_t i = 0; i < pri.size(); ++i)
    if (pri[i] < prior_cutoff) { pri[i] = prior_cutoff; mask[i] = FLT_MAX / 2; }
  if (blank_scale != 1.0 && !pri.empty()) pri[0] *= blank_scale;
  double sum = 0;
  for (double v : pri) sum += v;
  std::vector<float> out(pri.size());
  for (size_t i = 0; i < pri.size(); ++i) out[i] = (float)std::log(pri[i] / sum) + mask[i];
  return out;
}

