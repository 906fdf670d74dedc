// labels/gnx_label_io.cpp — the .lai and .bed writers, host code only: gnx_write_lai / gnx_write_bed of include/gnomix_io.h, next to
// gnx_write_msp / gnx_write_fb of gnx_io.cpp, whose pool (gnx_io_parallel), thread counts and error slot they share.
//
// Reference: msp_to_lai (src/postprocess.py:128-160) repeats every .msp row once per SNP of its window through a DataFrame;
// msp_to_bed / get_bed_data (:162-210) walk every haplotype column of the .msp.  Both re-read the .msp text; these take the labels.
//
// .lai: a window's N labels are the same text for every one of its SNPs, so each window's line body ("\t<label>" x N, "\n") is
// formatted once and a line is the position plus a memcpy.  The lines are cut into blocks of at most kLaiBlockBytes of one window's
// SNPs; a group of blocks is formatted by the pool's threads while the calling thread writes the group before it (two sets of
// buffers, ONE writer, plain write(): what gnx_io.cpp measured as the fastest way into the page cache).
// .bed: one file per haplotype from the run list of gnx_label_runs and the .msp's column strings, one file per thread at a time.
#include "../gnx_io.h"

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <charconv>
#include <cstring>
#include <mutex>

namespace {

const int64_t kLaiBlockBytes = (int64_t)4 << 20;

inline int io_fail(int code, const std::string& msg) { return gnx_io_fail(code, msg); }

inline char* put_int(char* o, int64_t v) { return std::to_chars(o, o + 24, v).ptr; }

// dynamic loop over [0, n): body(i, tid), tid < min(n, n_threads)
template <class F>
void par_for(int64_t n, int n_threads, F&& body) {
  if (n <= 0) return;
  std::atomic<int64_t> next{0};
  gnx_io_parallel((int)std::min<int64_t>(n, n_threads), [&](int tid) {
    for (int64_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < n;) body(i, tid);
  });
}

bool put_all(int fd, const char* b, size_t n) {
  while (n > 0) {
    const ssize_t w = write(fd, b, n);
    if (w < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    b += w;
    n -= (size_t)w;
  }
  return true;
}

}  // namespace

extern "C" int gnx_write_lai(const char* path, const char* head, int64_t head_len, const int64_t* positions, int64_t n_positions,
                             const int64_t* n_snps, const int32_t* labels, int64_t N, int64_t ldl, int64_t W, int n_threads) {
  if (!path || head_len < 0 || (head_len > 0 && !head) || N < 0 || W < 0 || ldl < W || n_positions < 0 || (W > 0 && !n_snps) ||
      (n_positions > 0 && !positions) || (N > 0 && W > 0 && !labels))
    return io_fail(GNX_EINVAL, "write_lai: bad arguments");
  int64_t sum = 0;
  for (int64_t w = 0; w < W; ++w) {
    if (n_snps[w] < 0 || n_snps[w] > n_positions)
      return io_fail(GNX_EINVAL, "write_lai: window " + std::to_string(w) + " has a SNP count outside [0, len(positions)]");
    sum += n_snps[w];
  }
  if (sum != n_positions)  // the reference's assert np.sum(n_reps) == len(positions)
    return io_fail(GNX_EINVAL, "write_lai: the windows' SNP counts add up to " + std::to_string(sum) + ", the query has " +
                                   std::to_string(n_positions) + " positions");
  const int nt = gnx_io_stream_threads(n_threads);
  // every window's line body, once
  std::vector<std::vector<char>> body((size_t)W);
  par_for(W, nt, [&](int64_t w, int) {
    std::vector<char>& b = body[(size_t)w];
    b.resize((size_t)N * 12 + 2);
    char* o = b.data();
    for (int64_t n = 0; n < N; ++n) {
      *o++ = '\t';
      const int32_t v = labels[(size_t)n * ldl + w];
      if (v >= 0 && v < 10) *o++ = (char)('0' + v);
      else o = put_int(o, v);
    }
    if (N == 0) *o++ = '\t';  // the position's own separator: a line is position, tab, the joined labels
    *o++ = '\n';
    b.resize((size_t)(o - b.data()));
  });
  struct Block {
    int64_t w, p0, p1;  // SNPs p0 .. p1 - 1 of the query, all of window w
  };
  std::vector<Block> blocks;
  int64_t p = 0;
  for (int64_t w = 0; w < W; ++w) {
    const int64_t line = (int64_t)body[(size_t)w].size() + 20, per = std::max<int64_t>(1, kLaiBlockBytes / line);
    for (int64_t s = 0; s < n_snps[w]; s += per) blocks.push_back({w, p + s, p + std::min(n_snps[w], s + per)});
    p += n_snps[w];
  }
  auto format = [&](const Block& k, std::vector<char>& buf) {
    const std::vector<char>& b = body[(size_t)k.w];
    buf.resize((size_t)(k.p1 - k.p0) * (b.size() + 20));
    char* o = buf.data();
    for (int64_t q = k.p0; q < k.p1; ++q) {
      o = put_int(o, positions[q]);
      memcpy(o, b.data(), b.size());
      o += b.size();
    }
    buf.resize((size_t)(o - buf.data()));
  };
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return io_fail(GNX_EINVAL, std::string("write: cannot open ") + path + ": " + strerror(errno));
  bool ok = put_all(fd, head, (size_t)head_len);
  int err_no = ok ? 0 : errno;
  const int64_t nb = (int64_t)blocks.size();
  const int64_t G = nt > 1 ? 2 * (nt - 1) : 1;  // blocks per group
  std::vector<std::vector<char>> sets[2] = {std::vector<std::vector<char>>((size_t)G), std::vector<std::vector<char>>((size_t)G)};
  // step g: the workers format group g into sets[g % 2] while this thread writes group g - 1 out of the other set
  for (int64_t g = 0; ok && g * G < nb + G; ++g) {
    const int64_t f0 = g * G, f1 = std::min(nb, f0 + G), w0 = f0 - G, w1 = std::min(nb, f0);
    std::atomic<int64_t> next{f0};
    auto produce = [&] {
      for (int64_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < f1;) format(blocks[(size_t)i], sets[g % 2][(size_t)(i - f0)]);
    };
    auto drain = [&] {
      for (int64_t i = std::max<int64_t>(w0, 0); i < w1 && ok; ++i) {
        const std::vector<char>& buf = sets[(g + 1) % 2][(size_t)(i - w0)];
        if (!put_all(fd, buf.data(), buf.size())) {  // reported below; nothing waits on a failed write
          err_no = errno;
          ok = false;
        }
      }
    };
    if (nt == 1) {
      drain();
      produce();
    } else {
      gnx_io_parallel(nt, [&](int tid) {
        if (tid == 0) drain();
        else produce();
      });
    }
  }
  const int cr = close(fd);
  if (!ok || cr != 0) return io_fail(GNX_EINVAL, std::string("write: I/O error on ") + path + ": " + strerror(err_no ? err_no : errno));
  return GNX_OK;
}

extern "C" int gnx_write_bed(const char* dir, const char* file_blob, const int64_t* file_off, const char* head, int64_t head_len,
                             const char* col_blob, const int64_t* col_off, const char* anc_blob, const int64_t* anc_off, int64_t n_anc,
                             const int64_t* run_off, const int32_t* triples, int64_t N, int64_t W, int n_threads) {
  if (!dir || N < 0 || W < 0 || head_len < 0 || (head_len > 0 && !head) || n_anc < 0 || (n_anc > 0 && (!anc_blob || !anc_off)) ||
      (N > 0 && (!file_blob || !file_off || !run_off)) || (W > 0 && (!col_blob || !col_off)))
    return io_fail(GNX_EINVAL, "write_bed: bad arguments");
  for (int64_t n = 0; n < N; ++n)
    if (run_off[n + 1] < run_off[n] || run_off[n] < 0 || (run_off[n + 1] > run_off[n] && !triples))
      return io_fail(GNX_EINVAL, "write_bed: the runs' offsets must not decrease");
  std::mutex mu;
  std::string first_err;
  std::atomic<int> failed{0};
  auto fail_with = [&](const std::string& msg) {
    std::lock_guard<std::mutex> lk(mu);
    if (!failed.exchange(1)) first_err = msg;
  };
  auto col = [&](int64_t w, int c, std::vector<char>& buf) {
    buf.insert(buf.end(), col_blob + col_off[5 * w + c], col_blob + col_off[5 * w + c + 1]);
    buf.push_back('\t');
  };
  std::vector<std::vector<char>> bufs((size_t)std::max(1, gnx_io_stream_threads(n_threads)));  // the bound of the pool used here
  par_for(N, (int)bufs.size(), [&](int64_t n, int tid) {
    if (failed.load(std::memory_order_relaxed)) return;  // a failed file ends the job: the rest is skipped, nothing waits
    std::vector<char>& buf = bufs[(size_t)tid];
    buf.clear();
    for (int64_t r = run_off[n]; r < run_off[n + 1]; ++r) {
      const int64_t first = triples[3 * r], last = triples[3 * r + 1], lab = triples[3 * r + 2];
      if (first < 0 || last < first || last >= W)
        return fail_with("write_bed: run " + std::to_string(r) + " lies outside the " + std::to_string(W) + " windows");
      if (n_anc > 0 && (lab < 0 || lab >= n_anc))
        return fail_with("write_bed: label " + std::to_string(lab) + " has no name among the " + std::to_string(n_anc) + " populations");
      col(first, 0, buf);
      col(first, 1, buf);
      col(last, 2, buf);
      if (n_anc > 0) buf.insert(buf.end(), anc_blob + anc_off[lab], anc_blob + anc_off[lab + 1]);
      else {
        char tmp[24];
        buf.insert(buf.end(), tmp, put_int(tmp, lab));
      }
      buf.push_back('\t');
      col(first, 3, buf);
      col(last, 4, buf);
      buf.back() = '\n';
    }
    const std::string path = std::string(dir) + "/" + std::string(file_blob + file_off[n], (size_t)(file_off[n + 1] - file_off[n]));
    if (gnx_io_write_file(path.c_str(), head, (size_t)head_len, buf.data(), buf.size()) != GNX_OK) fail_with(gnx_io_last_error());
  });
  if (failed.load()) return io_fail(GNX_EINVAL, first_err);
  return GNX_OK;
}
