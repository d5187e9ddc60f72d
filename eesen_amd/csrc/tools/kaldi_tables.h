// kaldi_tables.h -- the Kaldi table formats the two tools read and write, in plain host C++ (shared by
// train_ctc_parallel.cc and net_output_extract.cc).  Formats follow the reference: archive entry = key + space + object
// (src/util/kaldi-table-inl.h), binary objects start with \0B (src/base/io-funcs-inl.h:183-187), float matrix FM
// (src/cpucompute/matrix.cc:968-994), compressed CM / CM2 (src/cpucompute/compressed-matrix.cc:437-520), int32 vectors
// (src/util/kaldi-holder-inl.h:190-260), script files `key path[:offset]` (src/util/kaldi-table.h), and RIFF/WAVE files with 16-bit
// PCM samples (src/feat/wave-reader.cc) for the tools that start at the audio.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ext/stdio_filebuf.h>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <memory>
#include <vector>

namespace ktab {

// The "extended filenames" of src/util/kaldi-io.cc that the recipes use: a plain path, `-` (stdin / stdout), `cmd |` (read
// the command's output) and `| cmd` (write into the command) -- steps/train_ctc_parallel.sh:95-115 always hands the
// trainer `ark,s,cs:apply-cmvn ... |` and `ark:gunzip -c labels.tr.gz|`, the decoding scripts pipe `net-output-extract ... ark:-`.
class InStream {
 public:
  explicit InStream(const std::string& xname) {
    std::string n = xname;
    while (!n.empty() && n.back() == ' ') n.pop_back();
    if (n == "-") { is_ = &std::cin; return; }
    if (!n.empty() && n.back() == '|') {
      n.pop_back();
      cmd_ = n;
      pipe_ = popen(n.c_str(), "r");
      if (!pipe_) throw std::runtime_error("cannot run '" + n + "'");
      buf_.reset(new __gnu_cxx::stdio_filebuf<char>(pipe_, std::ios::in | std::ios::binary));
      own_.reset(new std::istream(buf_.get()));
      is_ = own_.get();
      return;
    }
    auto f = new std::ifstream(n, std::ios::binary);
    own_.reset(f);
    if (!*f) throw std::runtime_error("cannot open " + n);
    is_ = f;
  }
  // A filter that failed leaves a TRUNCATED table behind an ordinary end-of-file (the reference warns, util/kaldi-io.cc
  // PipeInputImpl::Close; the Python reader raises): say so as soon as the stream is closed.
  ~InStream() {
    own_.reset(); buf_.reset();
    if (pipe_) {
      const int st = pclose(pipe_);
      if (st != 0) std::cerr << "WARNING (kaldi_tables) pipe '" << cmd_ << "' ended with status " << st << ": the table may be truncated" << std::endl;
    }
  }
  // to be called once the reader has hit end-of-file on a pipe it must be able to trust (feature and label tables of a trainer)
  void CloseChecked() {
    own_.reset(); buf_.reset();
    if (pipe_) {
      const int st = pclose(pipe_);
      pipe_ = nullptr;
      if (st != 0) throw std::runtime_error("pipe '" + cmd_ + "' ended with status " + std::to_string(st) + ": the table it produced is truncated");
    }
  }
  InStream(const InStream&) = delete;
  std::istream& get() { return *is_; }
 private:
  std::string cmd_;
  std::istream* is_ = nullptr;
  std::unique_ptr<std::istream> own_;
  std::unique_ptr<__gnu_cxx::stdio_filebuf<char>> buf_;
  FILE* pipe_ = nullptr;
};
class OutStream {
 public:
  explicit OutStream(const std::string& xname) {
    std::string n = xname;
    if (n == "-") { os_ = &std::cout; return; }
    if (!n.empty() && n.front() == '|') {
      pipe_ = popen(n.c_str() + 1, "w");
      if (!pipe_) throw std::runtime_error("cannot run '" + n.substr(1) + "'");
      buf_.reset(new __gnu_cxx::stdio_filebuf<char>(pipe_, std::ios::out | std::ios::binary));
      own_.reset(new std::ostream(buf_.get()));
      os_ = own_.get();
      return;
    }
    auto f = new std::ofstream(n, std::ios::binary);
    own_.reset(f);
    if (!*f) throw std::runtime_error("cannot open " + n + " for writing");
    os_ = f;
  }
  ~OutStream() {
    if (os_) os_->flush();
    own_.reset(); buf_.reset();
    if (pipe_) {
      const int st = pclose(pipe_);
      if (st != 0) std::cerr << "WARNING (kaldi_tables) output pipe ended with status " << st << std::endl;
    }
  }
  OutStream(const OutStream&) = delete;
  std::ostream& get() { return *os_; }
 private:
  std::ostream* os_ = nullptr;
  std::unique_ptr<std::ostream> own_;
  std::unique_ptr<__gnu_cxx::stdio_filebuf<char>> buf_;
  FILE* pipe_ = nullptr;
};

struct Mat {
  std::vector<float> v;
  int rows = 0, cols = 0;
};

inline void need(std::istream& is, const char* what) {
  if (!is) throw std::runtime_error(std::string("table read error: ") + what);
}
inline int32_t read_sized_int(std::istream& is) {  // io-funcs-inl.h:32-41: size byte 4 + little-endian payload
  char sz = 0;
  is.get(sz);
  int32_t v = 0;
  is.read(reinterpret_cast<char*>(&v), 4);
  if (!is || sz != 4) throw std::runtime_error("bad binary int32 in table");
  return v;
}
inline std::string read_key(std::istream& is) {  // bytes up to the first space; "" at EOF; leading newlines skipped (text mode)
  std::string k;
  char c;
  while (is.get(c)) {
    if (c == ' ' || c == '\t') { if (!k.empty()) return k; continue; }
    if ((c == '\n' || c == '\r') && k.empty()) continue;
    k.push_back(c);
  }
  return k;
}
inline float u16_to_float(float min_value, float range, uint16_t v) {  // compressed-matrix.cc:244-250
  return min_value + range * 1.52590218966964e-05F * v;
}
inline float char_to_float(float p0, float p25, float p75, float p100, unsigned char value) {  // compressed-matrix.cc:363-373
  if (value <= 64) return p0 + (p25 - p0) * value * (1 / 64.0);
  if (value <= 192) return p25 + (p75 - p25) * (value - 64) * (1 / 128.0);
  return p75 + (p100 - p75) * (value - 192) * (1 / 63.0);
}
inline Mat read_compressed(std::istream& is, int format) {  // compressed-matrix.cc:437-470 + CopyToMat :485-520
  struct { float min_value, range; int32_t num_rows, num_cols; } h;
  is.read(reinterpret_cast<char*>(&h), sizeof(h));
  need(is, "compressed-matrix header");
  Mat m;
  m.rows = h.num_rows; m.cols = h.num_cols;
  if (h.num_cols == 0) { m.rows = 0; return m; }
  m.v.resize((size_t)m.rows * m.cols);
  if (format == 2) {
    std::vector<uint16_t> d((size_t)m.rows * m.cols);
    is.read(reinterpret_cast<char*>(d.data()), d.size() * 2);
    need(is, "CM2 data");
    for (size_t i = 0; i < d.size(); ++i) m.v[i] = u16_to_float(h.min_value, h.range, d[i]);
    return m;
  }
  std::vector<uint16_t> pc((size_t)4 * m.cols);
  is.read(reinterpret_cast<char*>(pc.data()), pc.size() * 2);
  std::vector<unsigned char> bytes((size_t)m.rows * m.cols);
  is.read(reinterpret_cast<char*>(bytes.data()), bytes.size());
  need(is, "CM data");
  for (int c = 0; c < m.cols; ++c) {
    const float p0 = u16_to_float(h.min_value, h.range, pc[4 * c]), p25 = u16_to_float(h.min_value, h.range, pc[4 * c + 1]),
                p75 = u16_to_float(h.min_value, h.range, pc[4 * c + 2]), p100 = u16_to_float(h.min_value, h.range, pc[4 * c + 3]);
    for (int r = 0; r < m.rows; ++r) m.v[(size_t)r * m.cols + c] = char_to_float(p0, p25, p75, p100, bytes[(size_t)c * m.rows + r]);
  }
  return m;
}
inline Mat read_matrix(std::istream& is) {
  Mat m;
  if (is.peek() == '\0') {  // binary: \0B then a token
    is.get(); is.get();
    std::string tok;
    is >> tok;
    is.get();  // the space after the token
    if (tok == "CM") return read_compressed(is, 1);
    if (tok == "CM2") return read_compressed(is, 2);
    if (tok == "DM") throw std::runtime_error("double-precision matrices are not supported (the path is BaseFloat = float)");
    if (tok != "FM") throw std::runtime_error("expected FM / CM / CM2, got " + tok);
    m.rows = read_sized_int(is); m.cols = read_sized_int(is);
    m.v.resize((size_t)m.rows * m.cols);
    is.read(reinterpret_cast<char*>(m.v.data()), m.v.size() * 4);
    need(is, "matrix data");
    return m;
  }
  // text: " [" rows separated by newlines "]"
  char c;
  do { need(is.get(c), "text matrix"); } while (c != '[');
  std::string body;
  std::getline(is, body, ']');
  std::istringstream rows(body);
  std::string line;
  while (std::getline(rows, line)) {
    std::istringstream ls(line);
    float f;
    int n = 0;
    while (ls >> f) { m.v.push_back(f); ++n; }
    if (n) { if (m.cols && n != m.cols) throw std::runtime_error("ragged text matrix"); m.cols = n; ++m.rows; }
  }
  std::getline(is, line);  // rest of the closing line
  return m;
}
inline std::vector<int32_t> read_int_vector(std::istream& is) {
  std::vector<int32_t> v;
  if (is.peek() == '\0') {
    is.get(); is.get();
    const int32_t n = read_sized_int(is);
    v.resize(n);
    for (int32_t i = 0; i < n; ++i) v[i] = read_sized_int(is);
    return v;
  }
  std::string line;
  std::getline(is, line);
  std::istringstream ls(line);
  int32_t x;
  while (ls >> x) v.push_back(x);
  return v;
}
// WaveData::Read (src/feat/wave-reader.cc) for what the recipes feed it: RIFF/WAVE, PCM (format 1), 16 bits per sample, any channel
// count -> [samples x channels] floats in int16 scale (the file's own interleaving) and the sample rate.  Chunks between `fmt ` and
// `data` are skipped; a data chunk size of 0 or 0xFFFFFFFF (what sox and ffmpeg write into a pipe) means "read to the end", and a
// data chunk cut short gives the samples that are there.  8- and 32-bit samples, RIFX and non-PCM formats are refused.
struct Wave { Mat data; float samp_freq = 0.f; };
inline Wave read_wave(std::istream& is) {
  auto rd = [&](void* dst, size_t n, const char* what) {
    is.read(static_cast<char*>(dst), (std::streamsize)n);
    if (!is) throw std::runtime_error(std::string("WaveData: unexpected end of file (") + what + ")");
  };
  auto u32 = [&](const char* what) { unsigned char b[4]; rd(b, 4, what); return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; };
  auto u16 = [&](const char* what) { unsigned char b[2]; rd(b, 2, what); return (uint32_t)b[0] | (uint32_t)b[1] << 8; };
  char tag[5] = {0, 0, 0, 0, 0};
  rd(tag, 4, "RIFF tag");
  if (std::strcmp(tag, "RIFF")) throw std::runtime_error(std::string("WaveData: expected RIFF, got ") + tag);
  u32("RIFF chunk size");
  rd(tag, 4, "WAVE tag");
  if (std::strcmp(tag, "WAVE")) throw std::runtime_error("WaveData: expected WAVE");
  rd(tag, 4, "fmt tag");
  if (std::strcmp(tag, "fmt ")) throw std::runtime_error("WaveData: expected the fmt chunk");
  const uint32_t fmt_size = u32("fmt chunk size");
  if (fmt_size < 16) throw std::runtime_error("WaveData: expect PCM format data to have fmt chunk of at least size 16.");
  const uint32_t audio_format = u16("fmt"), channels = u16("fmt"), rate = u32("fmt"), byte_rate = u32("fmt"), block_align = u16("fmt"), bits = u16("fmt");
  if (audio_format != 1) throw std::runtime_error("WaveData: can read only PCM data, format id in file is: " + std::to_string(audio_format));
  for (uint32_t i = 16; i < fmt_size; ++i) { char c; rd(&c, 1, "fmt chunk"); }
  if (channels == 0) throw std::runtime_error("WaveData: no channels present");
  if (bits != 16) throw std::runtime_error("WaveData: only 16-bit samples are supported, bits_per_sample is " + std::to_string(bits));
  if (byte_rate != rate * 2 * channels) throw std::runtime_error("Unexpected byte rate " + std::to_string(byte_rate) + " vs. " + std::to_string(rate) + " * 2 * " + std::to_string(channels));
  if (block_align != 2 * channels) throw std::runtime_error("Unexpected block_align: " + std::to_string(block_align) + " vs. " + std::to_string(channels) + " * 2");
  uint32_t size = 0;
  for (;;) {
    rd(tag, 4, "chunk name");
    size = u32("chunk size");
    if (!std::strcmp(tag, "data")) break;
    for (uint32_t i = 0; i < size; ++i) { char c; rd(&c, 1, "chunk"); }
  }
  std::string raw;
  if (size == 0 || size == 0xFFFFFFFFu) {
    raw.assign(std::istreambuf_iterator<char>(is), std::istreambuf_iterator<char>());
  } else {
    raw.resize(size);
    is.read(&raw[0], (std::streamsize)size);
    raw.resize((size_t)is.gcount());
    is.clear();
    if (raw.empty()) throw std::runtime_error("WaveData: failed to read data chunk (read no bytes)");
  }
  Wave w;
  w.samp_freq = (float)rate;
  w.data.cols = (int)channels;
  w.data.rows = (int)(raw.size() / block_align);
  w.data.v.resize((size_t)w.data.rows * channels);
  const unsigned char* b = reinterpret_cast<const unsigned char*>(raw.data());
  for (size_t i = 0; i < w.data.v.size(); ++i) w.data.v[i] = (float)(int16_t)((uint16_t)b[2 * i] | (uint16_t)b[2 * i + 1] << 8);
  return w;
}
// What compute-fbank-feats does with a wave file before the features (compute-fbank-feats.cc:97-139): a FeatureReader given one of
// these reads a wav table and yields the chosen channel as a [samples x 1] matrix.
struct WaveSelect { float samp_freq = 16000.f; int channel = -1; float min_duration = 0.f; std::string tool = "compute-fbank-feats"; };

struct Spec { std::string kind, path; };
inline Spec parse_spec(const std::string& s) {
  const size_t c = s.find(':');
  if (c == std::string::npos) throw std::runtime_error("bad table specifier '" + s + "' (expected ark:... or scp:...)");
  Spec sp{s.substr(0, s.find_first_of(",:")), s.substr(c + 1)};
  if (sp.kind != "ark" && sp.kind != "scp") throw std::runtime_error("unsupported table kind in '" + s + "'");
  return sp;
}
// `path[:offset]` of a script-file entry: the byte offset behind the last ':' when only digits follow it
inline std::streamoff split_scp_offset(std::string* loc) {
  const size_t c = loc->rfind(':');
  if (c == std::string::npos || c + 1 >= loc->size() || loc->find_first_not_of("0123456789", c + 1) != std::string::npos) return 0;
  const std::streamoff off = std::stoll(loc->substr(c + 1));
  *loc = loc->substr(0, c);
  return off;
}
// SequentialBaseFloatMatrixReader (train-ctc-parallel.cc:124)
class FeatureReader {
 public:
  explicit FeatureReader(const std::string& rspecifier, const WaveSelect* wave = nullptr)
      : sp_(parse_spec(rspecifier)), in_(sp_.path), f_(in_.get()), wave_(wave ? new WaveSelect(*wave) : nullptr) { Next(); }
  long NumRead() const { return num_read_; }   // table entries seen, skipped ones included
  bool Done() const { return done_; }
  const std::string& Key() const { return key_; }
  Mat& Value() { return val_; }
  void Next() {
    do { skip_ = false; Advance(); } while (!done_ && skip_);
  }
 private:
  // a matrix, or in wave mode the chosen channel of a wave file; skip_ is set for an utterance the tool writes nothing for
  Mat read_obj(std::istream& is) {
    ++num_read_;
    if (!wave_) return read_matrix(is);
    Wave w = read_wave(is);
    const std::string warn = "WARNING (" + wave_->tool + ":main()) ";
    const double dur = w.data.rows / (double)w.samp_freq;
    if (dur < wave_->min_duration) {
      std::cerr << warn << "File: " << key_ << " is too short (" << dur << " sec): producing no output." << std::endl;
      skip_ = true;
      return Mat();
    }
    const int nch = w.data.cols;
    int ch = wave_->channel;
    if (ch == -1) {
      ch = 0;
      if (nch != 1) std::cerr << warn << "Channel not specified but you have data with " << nch << " channels; defaulting to zero" << std::endl;
    } else if (ch >= nch) {
      std::cerr << warn << "File with id " << key_ << " has " << nch << " channels but you specified channel " << ch << ", producing no output." << std::endl;
      skip_ = true;
      return Mat();
    }
    if (w.samp_freq != wave_->samp_freq)
      throw std::runtime_error("Sample frequency mismatch: you specified " + std::to_string(wave_->samp_freq) + " but data has " + std::to_string(w.samp_freq) +
                               " (use --sample-frequency option).  Utterance is " + key_);
    Mat m;
    m.rows = w.data.rows; m.cols = 1;
    m.v.resize((size_t)m.rows);
    for (int i = 0; i < m.rows; ++i) m.v[i] = w.data.v[(size_t)i * nch + ch];
    return m;
  }
  void Advance() {
    if (done_) return;
    if (sp_.kind == "ark") {
      key_ = read_key(f_);
      if (key_.empty()) { done_ = true; in_.CloseChecked(); return; }
      val_ = read_obj(f_);
      return;
    }
    std::string line;
    while (std::getline(f_, line)) {
      // `key<whitespace>rest-of-line` (util/kaldi-table.cc ReadScriptFile): the entry is everything behind the first run of
      // whitespace that follows the key -- NOT the first occurrence of its first word, which may sit inside the key itself
      const size_t k0 = line.find_first_not_of(" \t");
      if (k0 == std::string::npos) continue;
      const size_t k1 = line.find_first_of(" \t", k0);
      if (k1 == std::string::npos) continue;
      const size_t r0 = line.find_first_not_of(" \t", k1);
      if (r0 == std::string::npos) continue;
      key_ = line.substr(k0, k1 - k0);
      const std::string whole = line.substr(r0);
      std::string loc = whole.substr(0, whole.find_first_of(" \t"));
      const std::streamoff off = split_scp_offset(&loc);
      // a script entry may itself be a command: `key cmd args |`
      if (!whole.empty() && whole.find_last_not_of(" \t") != std::string::npos && whole[whole.find_last_not_of(" \t")] == '|') {
        InStream a(whole);
        val_ = read_obj(a.get());
        return;
      }
      std::ifstream a(loc, std::ios::binary);
      if (!a) throw std::runtime_error("cannot open " + loc);
      a.seekg(off);
      val_ = read_obj(a);
      return;
    }
    done_ = true;
  }
  Spec sp_;
  InStream in_;
  std::istream& f_;
  std::unique_ptr<WaveSelect> wave_;
  std::string key_;
  Mat val_;
  bool done_ = false, skip_ = false;
  long num_read_ = 0;
};
// RandomAccessInt32VectorReader (train-ctc-parallel.cc:125): the whole table in memory
inline std::map<std::string, std::vector<int32_t>> read_targets(const std::string& rspecifier) {
  const Spec sp = parse_spec(rspecifier);
  if (sp.kind != "ark") throw std::runtime_error("labels: only ark: tables are supported");
  InStream in(sp.path);
  std::istream& f = in.get();
  std::map<std::string, std::vector<int32_t>> t;
  for (;;) {
    const std::string k = read_key(f);
    if (k.empty()) break;
    t[k] = read_int_vector(f);
  }
  in.CloseChecked();   // `ark:gunzip -c labels.tr.gz|` that failed must not leave the trainer with half the transcripts
  return t;
}


// What the matrix writers share: `ark:file` (binary), `ark,t:file` (text) or `ark,scp:file.ark,file.scp` (the archive and a script of
// `key file.ark:offset` lines, the offset pointing at the object behind the key)
class TableWriterBase {
 public:
  explicit TableWriterBase(const std::string& wspecifier) {
    const size_t colon = wspecifier.find(':');
    if (colon == std::string::npos) throw std::runtime_error("bad table specifier '" + wspecifier + "' (expected ark:... or ark,scp:...)");
    std::vector<std::string> opts;
    std::istringstream hs(wspecifier.substr(0, colon));
    for (std::string o; std::getline(hs, o, ',');) opts.push_back(o);
    int i_ark = -1, i_scp = -1;
    for (size_t i = 0; i < opts.size(); ++i) { if (opts[i] == "ark") i_ark = (int)i; if (opts[i] == "scp") i_scp = (int)i; if (opts[i] == "t") text_ = true; }
    if (i_ark < 0) throw std::runtime_error("only ark: output is supported");
    std::string path = wspecifier.substr(colon + 1);
    if (i_scp >= 0) {
      const size_t comma = path.find(',');
      if (comma == std::string::npos) throw std::runtime_error("wspecifier '" + wspecifier + "' names one file for an archive and a script");
      std::string a = path.substr(0, comma), b = path.substr(comma + 1);
      if (i_scp < i_ark) std::swap(a, b);
      path = a;
      scp_.reset(new std::ofstream(b));
      if (!*scp_) throw std::runtime_error("cannot open " + b + " for writing");
    }
    ark_path_ = path;
    out_.reset(new OutStream(path));
  }
 protected:
  std::ostream& Begin(const std::string& key) {   // the script line and `key `: the object follows
    std::ostream& f_ = out_->get();
    if (scp_) {   // the offset points behind `key `; text entries have no fixed size, so the stream says how far it got
      *scp_ << key << ' ' << ark_path_ << ':' << (long)f_.tellp() + (long)key.size() + 1 << "\n";
      scp_->flush();
    }
    f_ << key << ' ';
    return f_;
  }
  static void End(std::ostream& f_) {
    f_.flush();   // every utterance leaves at once: downstream tools of a pipe (`... ark:- | latgen-faster ...`) start on it
    if (!f_) throw std::runtime_error("write error");
  }
  std::unique_ptr<OutStream> out_;
  std::unique_ptr<std::ofstream> scp_;
  std::string ark_path_;
  bool text_ = false;
};

// Matrix<Real>::Write (src/cpucompute/matrix.cc:1104-1140) behind the binary header: token FM / DM, the two sized ints, the rows; in
// text ` [`, one line per row, `]`
template <class Real>
inline void write_matrix_body(std::ostream& f_, bool text, const Real* data, int rows, int cols, int ld, int precision) {
  if (text) {
    f_ << " [";
    f_.precision(precision);
    for (int r = 0; r < rows; ++r) {
      f_ << "\n  ";
      for (int c = 0; c < cols; ++c) f_ << data[(size_t)r * ld + c] << ' ';
    }
    f_ << "]\n";
    return;
  }
  f_.write(sizeof(Real) == 8 ? "\0BDM " : "\0BFM ", 5);
  const char four = 4;
  const int32_t rc[2] = {rows, cols};
  for (int i = 0; i < 2; ++i) { f_.write(&four, 1); f_.write(reinterpret_cast<const char*>(&rc[i]), 4); }
  for (int r = 0; r < rows; ++r) f_.write(reinterpret_cast<const char*>(data + (size_t)r * ld), (size_t)cols * sizeof(Real));
}

// BaseFloatMatrixWriter
class MatrixWriter : public TableWriterBase {
 public:
  using TableWriterBase::TableWriterBase;
  void Write(const std::string& key, const float* data, int rows, int cols, int ld) {
    std::ostream& f_ = Begin(key);
    write_matrix_body(f_, text_, data, rows, cols, ld, 9);
    End(f_);
  }
};

// DoubleMatrixWriter (compute-cmvn-stats.cc:90): `DM` in binary; in text the reference's stream precision, 7 digits
// (InitKaldiOutputStream, src/base/io-funcs-inl.h:188-193)
class DoubleMatrixWriter : public TableWriterBase {
 public:
  using TableWriterBase::TableWriterBase;
  void Write(const std::string& key, const double* data, int rows, int cols) {
    std::ostream& f_ = Begin(key);
    write_matrix_body(f_, text_, data, rows, cols, cols, 7);
    End(f_);
  }
};

// Vector<BaseFloat>::Read (src/cpucompute/vector.cc): binary `FV ` + sized int + floats, text ` [ 1 2 3 ]`
inline std::vector<float> read_float_vector(std::istream& is) {
  std::vector<float> v;
  if (is.peek() == '\0') {
    is.get(); is.get();
    std::string tok;
    is >> tok;
    is.get();
    if (tok != "FV" && tok != "DV") throw std::runtime_error("expected FV or DV, got " + tok);
    const int32_t n = read_sized_int(is);
    if (n < 0) throw std::runtime_error("negative vector size in table");
    v.resize(n);
    if (tok == "FV") {
      is.read(reinterpret_cast<char*>(v.data()), (std::streamsize)n * 4);
    } else {
      std::vector<double> d(n);
      is.read(reinterpret_cast<char*>(d.data()), (std::streamsize)n * 8);
      for (int32_t i = 0; i < n; ++i) v[i] = (float)d[i];
    }
    need(is, "vector data");
    return v;
  }
  char c;
  do { need(is.get(c), "text vector"); } while (c != '[');
  std::string body;
  std::getline(is, body, ']');
  std::istringstream ls(body);
  float f;
  while (ls >> f) v.push_back(f);
  std::getline(is, body);  // rest of the closing line
  return v;
}
// key -> object of an `ark:` or `scp:` table read whole: read_obj(stream) reads one object
template <class T, class ReadObj>
inline void read_whole_table(const std::string& rspecifier, ReadObj read_obj, std::vector<std::pair<std::string, T>>* out) {
  const Spec sp = parse_spec(rspecifier);
  InStream in(sp.path);
  std::istream& f = in.get();
  if (sp.kind == "ark") {
    for (std::string key = read_key(f); !key.empty(); key = read_key(f)) out->emplace_back(key, read_obj(f));
    in.CloseChecked();
    return;
  }
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    std::string key, loc;
    if (!(ls >> key >> loc)) continue;
    const std::streamoff off = split_scp_offset(&loc);
    std::ifstream a(loc, std::ios::binary);
    if (!a) throw std::runtime_error("cannot open " + loc);
    a.seekg(off);
    out->emplace_back(key, read_obj(a));
  }
}
// RandomAccessBaseFloatVectorReader (compute-cmvn-stats.cc:84): the whole table in memory
inline std::map<std::string, std::vector<float>> read_float_vectors(const std::string& rspecifier) {
  std::vector<std::pair<std::string, std::vector<float>>> items;
  read_whole_table<std::vector<float>>(rspecifier, read_float_vector, &items);
  std::map<std::string, std::vector<float>> t;
  for (auto& kv : items) t[kv.first] = std::move(kv.second);
  return t;
}
// SequentialTokenVectorReader (compute-cmvn-stats.cc:93, TokenVectorHolder: one line of tokens per key): spk2utt, in file order
inline std::vector<std::pair<std::string, std::vector<std::string>>> read_token_lists(const std::string& rspecifier) {
  std::vector<std::pair<std::string, std::vector<std::string>>> out;
  read_whole_table<std::vector<std::string>>(rspecifier, [](std::istream& is) {
    std::string line;
    std::getline(is, line);
    std::istringstream ls(line);
    std::vector<std::string> toks;
    for (std::string t; ls >> t;) toks.push_back(t);
    return toks;
  }, &out);
  return out;
}

// Int32VectorWriter to `ark:file` (binary) or `ark,t:file` (text): what read_int_vector above and the trainers' target readers take
class IntVectorWriter {
 public:
  explicit IntVectorWriter(const std::string& wspecifier) {
    const Spec sp = parse_spec(wspecifier);
    if (sp.kind != "ark") throw std::runtime_error("only ark: output is supported");
    text_ = wspecifier.substr(0, wspecifier.find(':')).find(",t") != std::string::npos;
    out_.reset(new OutStream(sp.path));
  }
  void Write(const std::string& key, const int32_t* v, int n, int stride = 1) {
    std::ostream& f_ = out_->get();
    f_ << key << ' ';
    if (text_) {
      for (int i = 0; i < n; ++i) f_ << v[(size_t)i * stride] << ' ';
      f_ << '\n';
    } else {
      const char four = 4;
      const int32_t size = n;
      f_.write("\0B", 2);
      f_.write(&four, 1);
      f_.write(reinterpret_cast<const char*>(&size), 4);
      for (int i = 0; i < n; ++i) { f_.write(&four, 1); f_.write(reinterpret_cast<const char*>(v + (size_t)i * stride), 4); }
    }
    f_.flush();
    if (!f_) throw std::runtime_error("write error");
  }
 private:
  std::unique_ptr<OutStream> out_;
  bool text_ = false;
};

}  // namespace ktab
