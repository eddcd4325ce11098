/* Host check of csrc/init_proof_host.h under ASan + UBSan: a stand-alone
 * program, needs no GPU.  `make init_proof_host_test DIR=... TOTAL=...` runs
 * it over a dir of postdata_hits.part-* files (the CPU tests' parts, or an
 * init's): the merge and the winner rule as post_init_proof_assemble runs
 * them, then, on a private copy of every part, the truncation a resume does,
 * at every record boundary and inside every record, each time checked
 * against a fresh parse.  Exit status 0 when every check held. */
#include <cinttypes>

#include "../go-spacemesh_amd/csrc/init_proof_host.h"

using namespace initproof;

static int fails = 0;
#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);             \
      fails++;                                                                 \
    }                                                                          \
  } while (0)

static bool load(const std::string &path, std::vector<uint8_t> &raw) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  const bool ok = read_fd(fd, raw);
  (void)::close(fd);
  return ok;
}

/* one cut of one part: the file shortened to `bytes`, then resumed at
 * `point` */
static void resume_once(const std::vector<uint8_t> &raw, const Header &h,
                        uint64_t bytes, uint64_t point,
                        const std::string &scratch) {
  const int fd = ::open(scratch.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
  CHECK(fd >= 0);
  if (fd < 0) return;
  CHECK(write_at(fd, raw.data(), (size_t)bytes, 0));
  Body before;
  parse_body(raw.data() + HEADER_BYTES, bytes - HEADER_BYTES, h, before);
  uint64_t p = point, size = 0;
  std::string err;
  CHECK(sync_part(fd, h, &p, &size, err) == POST_OK);
  const uint64_t want =
      std::max(h.index_start, std::min(point, before.complete_to));
  CHECK(p == want);
  std::vector<uint8_t> now;
  CHECK(read_fd(fd, now) && now.size() == size);
  (void)::close(fd);
  if (now.size() < HEADER_BYTES) return;
  CHECK((now.size() - HEADER_BYTES) % RECORD_BYTES == 0);
  Body after;
  parse_body(now.data() + HEADER_BYTES, now.size() - HEADER_BYTES, h, after);
  CHECK(after.have_marker && after.complete_to == p);
  CHECK(after.good_bytes == now.size() - HEADER_BYTES);
  /* exactly the hits below the point survive, in order */
  size_t keep = 0;
  while (keep < before.hits.size() && before.hits[keep].index < p) keep++;
  CHECK(after.hits.size() == keep);
  for (size_t i = 0; i < keep && i < after.hits.size(); i++)
    CHECK(after.hits[i].index == before.hits[i].index &&
          after.hits[i].nonce == before.hits[i].nonce);
}

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s DIR TOTAL_LABELS\n", argv[0]);
    return 2;
  }
  const char *dir = argv[1];
  const uint64_t total = strtoull(argv[2], nullptr, 10);

  PostProof proof;
  PostInitProofReport rep;
  std::memset(&rep, 0, sizeof rep);
  std::string err;
  const int rc = assemble_dir(dir, total, &proof, &rep, err);
  if (rc == POST_OK)
    std::printf("assemble: nonce %u pow %" PRIu64 " indices %u B; %u parts, %"
                PRIu64 " hits over %" PRIu64 " labels\n",
                proof.nonce, proof.pow, proof.indices_len, rep.parts, rep.hits,
                rep.labels_covered);
  else
    std::printf("assemble: status %d: %s\n", rc, err.c_str());

  /* whatever the tiling says, every part that has a header is resumed */
  const char *tmp = getenv("TMPDIR");
  const std::string scratch = std::string(tmp && *tmp ? tmp : "/tmp") +
                              "/init_proof_host_test." +
                              std::to_string(getpid());
  DIR *dh = ::opendir(dir);
  CHECK(dh != nullptr);
  std::vector<std::string> names;
  while (dh) {
    struct dirent *de = ::readdir(dh);
    if (!de) break;
    if (std::strncmp(de->d_name, PREFIX, sizeof PREFIX - 1) == 0)
      names.push_back(de->d_name);
  }
  if (dh) ::closedir(dh);
  uint64_t cuts = 0;
  for (const std::string &name : names) {
    std::vector<uint8_t> raw;
    Header h;
    if (!load(std::string(dir) + "/" + name, raw) ||
        raw.size() < HEADER_BYTES || !unpack_header(raw.data(), h) ||
        h.nonces == 0 || h.index_start >= h.index_end)
      continue;
    /* keep the program quick on a large part: a stride over the cuts */
    const uint64_t body = raw.size() - HEADER_BYTES;
    const uint64_t step = std::max<uint64_t>(1, body / 16 / 400) * 16;
    for (uint64_t b = 0; b <= body; b += step)
      for (uint64_t torn : {0u, 7u}) {
        if (b + torn > body) continue;
        const uint64_t bytes = HEADER_BYTES + b + torn;
        for (uint64_t point :
             {h.index_start, (h.index_start + h.index_end) / 2, h.index_end,
              h.index_end + 5})
          resume_once(raw, h, bytes, point, scratch), cuts++;
      }
  }
  (void)::unlink(scratch.c_str());
  std::printf("resume: %" PRIu64 " cuts over %zu parts, %d checks failed\n",
              cuts, names.size(), fails);
  return fails ? 1 : 0;
}
