/* init_proof_host.h — the host half of "initial proof during init" (DESIGN
 * 3.8): the part-file format, its parser, the truncation a resume does, the
 * merge of the parts of a dir, and the winner rule shared with prove_core.
 * No HIP in here: engine.cpp includes it, and so does the stand-alone
 * sanitizer program tools/init_proof_host_test.cpp.
 *
 *   postdata_hits.part-<index_start>, little-endian
 *   header  128 bytes: magic PSTHITSP, u32 record_bytes = 16, u32 nonces,
 *           u32 k1, u32 k2, challenge[32], pow_difficulty[32],
 *           u64 index_start, u64 index_end, u64 total_labels, zeros
 *   records 16 bytes {u64 index, u32 nonce, u32 tag}: a hit has tag 0; a
 *           marker has nonce 0xFFFFFFFF, tag 0x4B52414D and index = the
 *           global index up to which the part is complete
 *
 * Well-formed means ascending: hits by (index, nonce), each at or behind the
 * marker in front of it and below index_end; a marker at or behind the one
 * before, above every hit in front of it, at most index_end.  What follows
 * the last well-formed marker does not count. */
#ifndef POSTE_INIT_PROOF_HOST_H
#define POSTE_INIT_PROOF_HOST_H

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spacemesh_post.h"
#include "crypto_host.h"
#include "post_common.h"

namespace initproof {

constexpr uint64_t HEADER_BYTES = 128;
constexpr uint64_t RECORD_BYTES = 16;
constexpr uint32_t MARK_NONCE = 0xFFFFFFFFu;
constexpr uint32_t MARK_TAG = 0x4B52414Du;
static const char MAGIC[8] = {'P', 'S', 'T', 'H', 'I', 'T', 'S', 'P'};
static const char PREFIX[] = "postdata_hits.part-";

inline void put_le(uint8_t *p, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t get_le(const uint8_t *p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

struct Header {
  uint32_t record_bytes = RECORD_BYTES, nonces = 0, k1 = 0, k2 = 0;
  uint8_t challenge[32] = {0}, pow_difficulty[32] = {0};
  uint64_t index_start = 0, index_end = 0, total_labels = 0;
};

inline void pack_header(const Header &h, uint8_t out[HEADER_BYTES]) {
  std::memset(out, 0, HEADER_BYTES);
  std::memcpy(out, MAGIC, 8);
  put_le(out + 8, h.record_bytes, 4);
  put_le(out + 12, h.nonces, 4);
  put_le(out + 16, h.k1, 4);
  put_le(out + 20, h.k2, 4);
  std::memcpy(out + 24, h.challenge, 32);
  std::memcpy(out + 56, h.pow_difficulty, 32);
  put_le(out + 88, h.index_start, 8);
  put_le(out + 96, h.index_end, 8);
  put_le(out + 104, h.total_labels, 8);
}

/* false for a wrong magic; the fields are not judged here */
inline bool unpack_header(const uint8_t *p, Header &h) {
  if (std::memcmp(p, MAGIC, 8) != 0) return false;
  h.record_bytes = (uint32_t)get_le(p + 8, 4);
  h.nonces = (uint32_t)get_le(p + 12, 4);
  h.k1 = (uint32_t)get_le(p + 16, 4);
  h.k2 = (uint32_t)get_le(p + 20, 4);
  std::memcpy(h.challenge, p + 24, 32);
  std::memcpy(h.pow_difficulty, p + 56, 32);
  h.index_start = get_le(p + 88, 8);
  h.index_end = get_le(p + 96, 8);
  h.total_labels = get_le(p + 104, 8);
  return true;
}

inline void pack_record(uint64_t index, uint32_t nonce, uint32_t tag,
                        uint8_t out[RECORD_BYTES]) {
  put_le(out, index, 8);
  put_le(out + 8, nonce, 4);
  put_le(out + 12, tag, 4);
}

inline std::string part_path(const std::string &dir, uint64_t start) {
  return dir + "/" + PREFIX + std::to_string(start);
}

/* The records of a part as far as they are well-formed. */
struct Body {
  std::vector<PostScanHit> hits; /* in front of the last marker */
  bool have_marker = false;
  uint64_t complete_to = 0;      /* the last marker's index; index_start
                                    while there is none */
  uint64_t good_bytes = 0;       /* body bytes up to and with that marker */
};

inline void parse_body(const uint8_t *body, uint64_t bytes, const Header &h,
                       Body &out) {
  out = Body();
  out.complete_to = h.index_start;
  size_t committed = 0;
  bool any_hit = false;
  uint64_t hit_index = 0;
  uint32_t hit_nonce = 0;
  for (uint64_t off = 0; off + RECORD_BYTES <= bytes; off += RECORD_BYTES) {
    const uint64_t index = get_le(body + off, 8);
    const uint32_t nonce = (uint32_t)get_le(body + off + 8, 4);
    const uint32_t tag = (uint32_t)get_le(body + off + 12, 4);
    if (nonce == MARK_NONCE && tag == MARK_TAG) {
      if (index < out.complete_to || index > h.index_end ||
          (any_hit && index <= hit_index))
        break;
      out.have_marker = true;
      out.complete_to = index;
      out.good_bytes = off + RECORD_BYTES;
      committed = out.hits.size();
    } else {
      if (tag != 0 || nonce >= h.nonces || index < out.complete_to ||
          index >= h.index_end)
        break;
      if (any_hit && (index < hit_index ||
                      (index == hit_index && nonce <= hit_nonce)))
        break;
      any_hit = true;
      hit_index = index;
      hit_nonce = nonce;
      PostScanHit hit;
      hit.index = index;
      hit.nonce = nonce;
      hit.pad = 0;
      out.hits.push_back(hit);
    }
  }
  out.hits.resize(committed);
}

/* body offset of the first well-formed record at or past `point` */
inline uint64_t cut_offset(const uint8_t *body, const Body &b,
                           uint64_t point) {
  for (uint64_t off = 0; off < b.good_bytes; off += RECORD_BYTES)
    if (get_le(body + off, 8) >= point) return off;
  return b.good_bytes;
}

inline bool read_fd(int fd, std::vector<uint8_t> &out) {
  struct stat st;
  if (::fstat(fd, &st) != 0) return false;
  out.resize((size_t)st.st_size);
  size_t got = 0;
  while (got < out.size()) {
    const ssize_t r = ::pread(fd, out.data() + got, out.size() - got,
                              (off_t)got);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    got += (size_t)r;
  }
  return true;
}

inline bool write_at(int fd, const uint8_t *p, size_t n, uint64_t at) {
  size_t put = 0;
  while (put < n) {
    const ssize_t w = ::pwrite(fd, p + put, n - put, (off_t)(at + put));
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    put += (size_t)w;
  }
  return true;
}

/* Bring an open part (header already checked) to a resume point: the point
 * is lowered to the last well-formed marker, the file is cut at the first
 * record at or past it, and a marker is written there.  *point is global;
 * *size receives the file's size afterwards. */
inline int sync_part(int fd, const Header &h, uint64_t *point, uint64_t *size,
                     std::string &err) {
  std::vector<uint8_t> raw;
  if (!read_fd(fd, raw) || raw.size() < HEADER_BYTES) {
    err = "cannot read the hits part";
    return POST_ERR_IO;
  }
  const uint8_t *body = raw.data() + HEADER_BYTES;
  Body b;
  parse_body(body, raw.size() - HEADER_BYTES, h, b);
  const uint64_t p = std::max(h.index_start, std::min(*point, b.complete_to));
  const uint64_t cut = HEADER_BYTES + cut_offset(body, b, p);
  uint8_t mark[RECORD_BYTES];
  pack_record(p, MARK_NONCE, MARK_TAG, mark);
  if (::ftruncate(fd, (off_t)cut) != 0 ||
      !write_at(fd, mark, RECORD_BYTES, cut)) {
    err = "cannot truncate the hits part";
    return POST_ERR_IO;
  }
  *point = p;
  *size = cut + RECORD_BYTES;
  return POST_OK;
}

/* Winner of a hit list: the nonce whose k2-th smallest passing index is
 * smallest (streaming-order first across the ascending scan); tie -> lowest
 * nonce.  Shared by prove_core and the assembly of the parts. */
inline int choose_winner(const std::vector<PostScanHit> &hits, uint32_t nonces,
                         uint32_t k2, uint64_t num_labels,
                         const std::vector<uint64_t> &group_pow,
                         PostProof *out, std::vector<uint64_t> *winner,
                         std::string &err) {
  std::vector<std::vector<uint64_t>> per_nonce(nonces);
  for (const auto &h : hits)
    if (h.nonce < nonces) per_nonce[h.nonce].push_back(h.index);
  int64_t best_nonce = -1;
  uint64_t best_kth = UINT64_MAX;
  for (uint32_t nn = 0; nn < nonces; nn++) {
    auto &v = per_nonce[nn];
    if (k2 == 0 || v.size() < k2) continue;
    std::sort(v.begin(), v.end());
    uint64_t kth = v[k2 - 1];
    if (kth < best_kth) {
      best_kth = kth;
      best_nonce = nn;
    }
  }
  if (best_nonce < 0) {
    err = "no nonce reached k2 passing indices";
    return POST_ERR_NO_NONCE;
  }
  out->nonce = (uint32_t)best_nonce;
  out->pow = group_pow[best_nonce / POSTE_NONCE_GROUP];
  out->num_indices = (uint16_t)k2;
  uint32_t bpi = poste::bits_per_index(num_labels);
  out->indices_len = poste::pack_indices(per_nonce[best_nonce].data(), k2, bpi,
                                         out->indices, POST_MAX_INDICES_BYTES);
  if (!out->indices_len) {
    err = "indices exceed the 800-byte wire cap";
    return POST_ERR;
  }
  if (winner)
    winner->assign(per_nonce[best_nonce].begin(),
                   per_nonce[best_nonce].begin() + k2);
  return POST_OK;
}

struct Part {
  std::string name;
  Header h;
  Body b;
};

inline std::string labels_missing(uint64_t a, uint64_t b) {
  return "labels [" + std::to_string(a) + ", " + std::to_string(b) +
         ") are missing";
}

/* Read every postdata_hits.part-* of a dir and require the parts to agree
 * and to tile [0, total) completely.  Reads only. */
inline int load_parts(const char *data_dir, uint64_t total,
                      std::vector<Part> &parts, std::string &err) {
  const std::string dir(data_dir);
  auto fail = [&err](const std::string &msg) {
    err = msg;
    return POST_ERR_IO;
  };
  DIR *dh = ::opendir(data_dir);
  if (!dh) return fail("cannot list " + dir);
  std::vector<std::string> names;
  while (struct dirent *de = ::readdir(dh))
    if (std::strncmp(de->d_name, PREFIX, sizeof PREFIX - 1) == 0)
      names.push_back(de->d_name);
  ::closedir(dh);
  std::sort(names.begin(), names.end());
  for (const std::string &name : names) {
    const char *num = name.c_str() + sizeof PREFIX - 1;
    char *e = nullptr;
    errno = 0;
    const uint64_t start = strtoull(num, &e, 10);
    if (*num < '0' || *num > '9' || *e != 0 || errno != 0) continue;
    const std::string path = dir + "/" + name;
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail("cannot open " + path);
    std::vector<uint8_t> raw;
    const bool ok = read_fd(fd, raw);
    (void)::close(fd);
    if (!ok) return fail("cannot read " + path);
    if (raw.size() < HEADER_BYTES)
      return fail(name + " is shorter than its header");
    Part p;
    p.name = name;
    if (!unpack_header(raw.data(), p.h)) return fail(name + " has a wrong magic");
    if (p.h.record_bytes != RECORD_BYTES)
      return fail(name + " has an unsupported record_bytes");
    if (p.h.index_start != start)
      return fail(name + ": index_start " + std::to_string(p.h.index_start) +
                  " disagrees with the file name");
    if (p.h.nonces == 0 || p.h.nonces % POSTE_NONCE_GROUP != 0)
      return fail(name + ": nonces is not a positive multiple of 16");
    if (p.h.total_labels != total)
      return fail(name + ": total_labels " +
                  std::to_string(p.h.total_labels) + " is not the dir's " +
                  std::to_string(total));
    if (p.h.index_start >= p.h.index_end || p.h.index_end > total)
      return fail(name + ": labels [" + std::to_string(p.h.index_start) +
                  ", " + std::to_string(p.h.index_end) +
                  ") lie outside the dir's " + std::to_string(total));
    if ((raw.size() - HEADER_BYTES) % RECORD_BYTES != 0)
      return fail(name + " ends inside a record (torn write): its session "
                  "must resume before the parts can be assembled");
    parse_body(raw.data() + HEADER_BYTES, raw.size() - HEADER_BYTES, p.h,
               p.b);
    if (!parts.empty()) {
      const Header &a = parts[0].h;
      const char *what =
          a.k1 != p.h.k1 ? "k1"
          : a.k2 != p.h.k2 ? "k2"
          : a.nonces != p.h.nonces ? "nonces"
          : std::memcmp(a.challenge, p.h.challenge, 32) != 0 ? "challenge"
          : std::memcmp(a.pow_difficulty, p.h.pow_difficulty, 32) != 0
              ? "pow_difficulty"
              : nullptr;
      if (what)
        return fail(name + " differs from " + parts[0].name + " in " + what);
    }
    parts.push_back(std::move(p));
  }
  if (parts.empty())
    return fail("no postdata_hits.part-* in " + dir + ": " +
                labels_missing(0, total));
  std::sort(parts.begin(), parts.end(), [](const Part &a, const Part &b) {
    return a.h.index_start < b.h.index_start;
  });
  uint64_t next = 0;
  for (const Part &p : parts) {
    if (p.h.index_start > next)
      return fail("the parts leave a gap: " +
                  labels_missing(next, p.h.index_start));
    if (p.h.index_start < next)
      return fail("the parts overlap: labels [" +
                  std::to_string(p.h.index_start) + ", " +
                  std::to_string(std::min(next, p.h.index_end)) +
                  ") are in more than one");
    if (p.b.complete_to < p.h.index_end)
      return fail(p.name + " is short, its shard is not finished: " +
                  labels_missing(p.b.complete_to, p.h.index_end));
    next = p.h.index_end;
  }
  if (next < total)
    return fail("the parts leave a gap: " + labels_missing(next, total));
  return POST_OK;
}

/* Merge the parts of a dir of `total` labels and choose the winner. */
inline int assemble_dir(const char *data_dir, uint64_t total, PostProof *out,
                        PostInitProofReport *r, std::string &err) {
  std::vector<Part> parts;
  int rc = load_parts(data_dir, total, parts, err);
  if (rc != POST_OK) return rc;
  std::vector<PostScanHit> hits;
  uint64_t covered = 0;
  for (const Part &p : parts) {
    hits.insert(hits.end(), p.b.hits.begin(), p.b.hits.end());
    covered += p.h.index_end - p.h.index_start;
  }
  const Header &h = parts[0].h;
  std::vector<uint64_t> group_pow(h.nonces / POSTE_NONCE_GROUP);
  for (uint32_t g = 0; g < group_pow.size(); g++)
    group_pow[g] =
        poste::k2pow_search_blake3(h.challenge, g, h.pow_difficulty, 0);
  if (r) {
    r->total_labels = total;
    r->labels_covered = covered;
    r->hits = hits.size();
    r->parts = (uint32_t)parts.size();
    r->reserved = 0;
  }
  std::memset(out, 0, sizeof *out);
  return choose_winner(hits, h.nonces, h.k2, total, group_pow, out, nullptr,
                       err);
}

} // namespace initproof

#endif
