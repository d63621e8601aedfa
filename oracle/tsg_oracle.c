/*
 * tsg_oracle.c — CPU ORACLE for the Tempo search path.  TEST INFRASTRUCTURE ONLY.
 *
 * Literal restatement of the reference Go code, function by function, each
 * citing the reference file:line it follows (paths relative to the reference
 * checkout). Deliberately written the way the reference executes it: per-search
 * snappy decode, flatbuffer pointer chasing, binary search over the descending
 * key vector, bytes.Contains over values. It is the parity checker for libtsg
 * and the CPU baseline in bench.py; it is never linked into the product.
 * Parity pinning: see tsg_oracle.h and tests/golden/README.md.
 */
#define _GNU_SOURCE
#include "tsg_oracle.h"

#include <ctype.h>
#include <dirent.h>
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

/* ------------------------------------------------------------------------- */
/* byte helpers (encoding/binary LittleEndian / BigEndian)                     */
static inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static inline uint32_t le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
static inline uint64_t be64(const uint8_t *p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
  return v;
}

void orc_free(void *p) { free(p); }

/* bytes.Compare */
static int bytes_compare(const uint8_t *a, size_t al, const uint8_t *b, size_t bl) {
  size_t n = al < bl ? al : bl;
  int c = n ? memcmp(a, b, n) : 0;
  if (c != 0) return c < 0 ? -1 : 1;
  if (al == bl) return 0;
  return al < bl ? -1 : 1;
}

/* bytes.Contains (an empty needle is contained in everything) */
static int bytes_contains(const uint8_t *h, size_t hl, const uint8_t *n, size_t nl) {
  if (nl == 0) return 1;
  if (nl > hl) return 0;
  for (size_t i = 0; i + nl <= hl; i++)
    if (h[i] == n[0] && memcmp(h + i, n, nl) == 0) return 1;
  return 0;
}

/* ------------------------------------------------------------------------- */
/* xxhash64, seed 0 (github.com/cespare/xxhash v1.1.0, Sum64 / Digest)         */
#define XP1 11400714785074694791ULL
#define XP2 14029467366897019727ULL
#define XP3 1609587929392839161ULL
#define XP4 9650029242287828579ULL
#define XP5 2870177450012600261ULL
static inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static inline uint64_t xround(uint64_t acc, uint64_t in) {
  acc += in * XP2;
  acc = rotl64(acc, 31);
  return acc * XP1;
}
static inline uint64_t xmerge(uint64_t acc, uint64_t v) {
  v = xround(0, v);
  acc ^= v;
  return acc * XP1 + XP4;
}
uint64_t orc_xxhash64(const uint8_t *p, size_t n) {
  const uint8_t *end = p + n;
  uint64_t h;
  if (n >= 32) {
    uint64_t v1 = XP1 + XP2, v2 = XP2, v3 = 0, v4 = (uint64_t)0 - XP1;
    while (end - p >= 32) {
      v1 = xround(v1, le64(p));
      v2 = xround(v2, le64(p + 8));
      v3 = xround(v3, le64(p + 16));
      v4 = xround(v4, le64(p + 24));
      p += 32;
    }
    h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    h = xmerge(h, v1);
    h = xmerge(h, v2);
    h = xmerge(h, v3);
    h = xmerge(h, v4);
  } else {
    h = XP5;
  }
  h += (uint64_t)n;
  while (end - p >= 8) {
    h ^= xround(0, le64(p));
    h = rotl64(h, 27) * XP1 + XP4;
    p += 8;
  }
  if (end - p >= 4) {
    h ^= (uint64_t)le32(p) * XP1;
    h = rotl64(h, 23) * XP2 + XP3;
    p += 4;
  }
  while (p < end) {
    h ^= (uint64_t)(*p) * XP5;
    h = rotl64(h, 11) * XP1;
    p++;
  }
  h ^= h >> 33;
  h *= XP2;
  h ^= h >> 29;
  h *= XP3;
  h ^= h >> 32;
  return h;
}

/* ------------------------------------------------------------------------- */
/* FNV-1 32 (hash/fnv New32) as used by util.TokenForTraceID (pkg/util/hash.go:15-20) */
uint32_t orc_fnv1_32(const uint8_t *p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; i++) {
    h *= 16777619u;
    h ^= p[i];
  }
  return h;
}

/* ------------------------------------------------------------------------- */
/* murmur3 x64 128, seed 0 (vendor/github.com/spaolacci/murmur3/murmur128.go:62-200) */
#define MC1 0x87c37b91114253d5ULL
#define MC2 0x4cf5ad432745937fULL
static inline uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}
void orc_murmur3_128(const uint8_t *p, size_t n, uint64_t out[2]) {
  uint64_t h1 = 0, h2 = 0;
  size_t nblocks = n / 16;
  for (size_t i = 0; i < nblocks; i++) {
    uint64_t k1 = le64(p + i * 16), k2 = le64(p + i * 16 + 8);
    k1 *= MC1; k1 = rotl64(k1, 31); k1 *= MC2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= MC2; k2 = rotl64(k2, 33); k2 *= MC1; h2 ^= k2;
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const uint8_t *t = p + nblocks * 16;
  uint64_t k1 = 0, k2 = 0;
  switch (n & 15) {
  case 15: k2 ^= (uint64_t)t[14] << 48; /* fallthrough */
  case 14: k2 ^= (uint64_t)t[13] << 40; /* fallthrough */
  case 13: k2 ^= (uint64_t)t[12] << 32; /* fallthrough */
  case 12: k2 ^= (uint64_t)t[11] << 24; /* fallthrough */
  case 11: k2 ^= (uint64_t)t[10] << 16; /* fallthrough */
  case 10: k2 ^= (uint64_t)t[9] << 8; /* fallthrough */
  case 9:
    k2 ^= (uint64_t)t[8];
    k2 *= MC2; k2 = rotl64(k2, 33); k2 *= MC1; h2 ^= k2;
    /* fallthrough */
  case 8: k1 ^= (uint64_t)t[7] << 56; /* fallthrough */
  case 7: k1 ^= (uint64_t)t[6] << 48; /* fallthrough */
  case 6: k1 ^= (uint64_t)t[5] << 40; /* fallthrough */
  case 5: k1 ^= (uint64_t)t[4] << 32; /* fallthrough */
  case 4: k1 ^= (uint64_t)t[3] << 24; /* fallthrough */
  case 3: k1 ^= (uint64_t)t[2] << 16; /* fallthrough */
  case 2: k1 ^= (uint64_t)t[1] << 8; /* fallthrough */
  case 1:
    k1 ^= (uint64_t)t[0];
    k1 *= MC1; k1 = rotl64(k1, 31); k1 *= MC2; h1 ^= k1;
  }
  h1 ^= (uint64_t)n;
  h2 ^= (uint64_t)n;
  h1 += h2;
  h2 += h1;
  h1 = fmix64(h1);
  h2 = fmix64(h2);
  h1 += h2;
  h2 += h1;
  out[0] = h1;
  out[1] = h2;
}

/* ------------------------------------------------------------------------- */
/* CRC-32C (Castagnoli) + snappy framing mask (vendor/github.com/golang/snappy/snappy.go:91-95) */
static uint32_t crc_tab[256];
static pthread_once_t crc_once = PTHREAD_ONCE_INIT;
static void crc_init(void) {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    crc_tab[i] = c;
  }
}
uint32_t orc_crc32c(const uint8_t *p, size_t n) {
  pthread_once(&crc_once, crc_init);
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) c = crc_tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
static uint32_t snappy_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

/* snappy block decode (vendor/github.com/golang/snappy/decode.go:27-75, decode_other.go:1-115) */
static int snappy_decoded_len(const uint8_t *src, size_t n, uint64_t *dlen, size_t *hlen) {
  uint64_t v = 0;
  int shift = 0;
  for (size_t i = 0; i < n && i < 10; i++) {
    uint8_t b = src[i];
    if (b < 0x80) {
      if (i == 9 && b > 1) return ORC_CORRUPT; /* overflow */
      v |= (uint64_t)b << shift;
      if (v > 0xffffffffULL) return ORC_CORRUPT;
      *dlen = v;
      *hlen = i + 1;
      return ORC_OK;
    }
    v |= (uint64_t)(b & 0x7f) << shift;
    shift += 7;
  }
  return ORC_CORRUPT;
}
static int snappy_decode_block(uint8_t *dst, size_t dlen, const uint8_t *src, size_t slen) {
  size_t d = 0, s = 0;
  while (s < slen) {
    size_t length = 0, offset = 0;
    uint8_t tag = src[s] & 3;
    if (tag == 0) {
      uint32_t x = src[s] >> 2;
      if (x < 60) {
        s += 1;
      } else {
        size_t nb = x - 59; /* 1..4 length bytes */
        s += 1 + nb;
        if (s > slen) return ORC_CORRUPT;
        x = 0;
        for (size_t i = 0; i < nb; i++) x |= (uint32_t)src[s - nb + i] << (8 * i);
      }
      length = (size_t)x + 1;
      if (length == 0) return ORC_CORRUPT;
      if (length > dlen - d || length > slen - s) return ORC_CORRUPT;
      memcpy(dst + d, src + s, length);
      d += length;
      s += length;
      continue;
    } else if (tag == 1) {
      s += 2;
      if (s > slen) return ORC_CORRUPT;
      length = 4 + ((src[s - 2] >> 2) & 7);
      offset = ((size_t)(src[s - 2] & 0xe0) << 3) | src[s - 1];
    } else if (tag == 2) {
      s += 3;
      if (s > slen) return ORC_CORRUPT;
      length = 1 + (src[s - 3] >> 2);
      offset = (size_t)src[s - 2] | ((size_t)src[s - 1] << 8);
    } else {
      s += 5;
      if (s > slen) return ORC_CORRUPT;
      length = 1 + (src[s - 5] >> 2);
      offset = (size_t)le32(src + s - 4);
    }
    if (offset == 0 || d < offset || length > dlen - d) return ORC_CORRUPT;
    for (size_t i = 0; i < length; i++) dst[d + i] = dst[d - offset + i]; /* forward copy */
    d += length;
  }
  return d == dlen ? ORC_OK : ORC_CORRUPT;
}

/* snappy.Reader.fill over a whole page (vendor/github.com/golang/snappy/decode.go:121-235):
 * first chunk must be the stream identifier; 0x00 compressed, 0x01 uncompressed,
 * both CRC32C-masked; 0x02-0x7f unsupported; 0x80-0xfe skipped. */
#define SNAPPY_MAX_BLOCK 65536
#define SNAPPY_MAX_ENC 76490
int orc_snappy_framed_decode(const uint8_t *src, size_t n, uint8_t **out, size_t *out_len) {
  size_t cap = 1 << 16, len = 0, s = 0;
  uint8_t *o = (uint8_t *)malloc(cap);
  uint8_t *blk = (uint8_t *)malloc(SNAPPY_MAX_BLOCK);
  int read_header = 0, rc = ORC_OK;
  const size_t buflen = SNAPPY_MAX_ENC + 4;
  while (s < n) {
    if (n - s < 4) { rc = ORC_CORRUPT; break; }
    uint8_t ct = src[s];
    size_t cl = (size_t)src[s + 1] | ((size_t)src[s + 2] << 8) | ((size_t)src[s + 3] << 16);
    s += 4;
    if (!read_header) {
      if (ct != 0xff) { rc = ORC_CORRUPT; break; }
      read_header = 1;
    }
    if (cl > buflen) { rc = ORC_CORRUPT; break; }
    if (cl > n - s) { rc = ORC_CORRUPT; break; }
    const uint8_t *body = src + s;
    s += cl;
    if (ct == 0x00 || ct == 0x01) {
      if (cl < 4) { rc = ORC_CORRUPT; break; }
      uint32_t csum = le32(body);
      const uint8_t *payload = body + 4;
      size_t pl = cl - 4;
      const uint8_t *dec;
      size_t dn;
      if (ct == 0x00) {
        uint64_t dl;
        size_t hl;
        if (snappy_decoded_len(payload, pl, &dl, &hl) != ORC_OK) { rc = ORC_CORRUPT; break; }
        if (dl > SNAPPY_MAX_BLOCK) { rc = ORC_CORRUPT; break; }
        if (snappy_decode_block(blk, (size_t)dl, payload + hl, pl - hl) != ORC_OK) { rc = ORC_CORRUPT; break; }
        dec = blk;
        dn = (size_t)dl;
      } else {
        if (pl > SNAPPY_MAX_BLOCK) { rc = ORC_CORRUPT; break; }
        dec = payload;
        dn = pl;
      }
      if (snappy_mask(orc_crc32c(dec, dn)) != csum) { rc = ORC_CORRUPT; break; }
      if (len + dn > cap) {
        while (len + dn > cap) cap *= 2;
        o = (uint8_t *)realloc(o, cap);
      }
      memcpy(o + len, dec, dn);
      len += dn;
    } else if (ct == 0xff) {
      if (cl != 6 || memcmp(body, "sNaPpY", 6) != 0) { rc = ORC_CORRUPT; break; }
    } else if (ct <= 0x7f) {
      rc = ORC_UNSUPPORTED_ENCODING;
      break;
    } /* else padding / skippable */
  }
  free(blk);
  if (rc != ORC_OK) {
    free(o);
    return rc;
  }
  *out = o;
  *out_len = len;
  return ORC_OK;
}

/* ------------------------------------------------------------------------- */
/* flatbuffers table access (vendor/github.com/google/flatbuffers/go/table.go:14-57) */
typedef struct fbt {
  const uint8_t *b;
  size_t n;
  uint32_t pos;
} fbt;
/* Bounds are checked so corrupt input cannot crash the checker; a well-formed
 * buffer reads exactly as table.go does. */
static int fb_ok(const fbt *t, uint64_t off, uint64_t len) { return off + len <= t->n; }
static uint16_t fb_offset(const fbt *t, uint16_t vto) {
  if (!fb_ok(t, t->pos, 4)) return 0;
  int32_t so = (int32_t)le32(t->b + t->pos);
  int64_t vt = (int64_t)t->pos - so;
  if (vt < 0 || !fb_ok(t, (uint64_t)vt, 2)) return 0;
  uint16_t vlen = le16(t->b + vt);
  if (vto < vlen && fb_ok(t, (uint64_t)vt + vto, 2)) return le16(t->b + vt + vto);
  return 0;
}
static uint32_t fb_indirect(const fbt *t, uint32_t off) {
  if (!fb_ok(t, off, 4)) return 0;
  return off + le32(t->b + off);
}
static uint32_t fb_vector(const fbt *t, uint16_t o) { /* start of vector data */
  uint32_t off = t->pos + o;
  return fb_indirect(t, off) + 4;
}
static uint32_t fb_vector_len(const fbt *t, uint16_t o) {
  uint32_t off = fb_indirect(t, t->pos + o);
  if (!fb_ok(t, off, 4)) return 0;
  return le32(t->b + off);
}
static const uint8_t *fb_byte_vector(const fbt *t, uint32_t off, uint32_t *len) {
  off = fb_indirect(t, off);
  if (!fb_ok(t, off, 4)) { *len = 0; return NULL; }
  uint32_t l = le32(t->b + off);
  if (!fb_ok(t, (uint64_t)off + 4, l)) { *len = 0; return NULL; }
  *len = l;
  return t->b + off + 4;
}
static fbt fb_root(const uint8_t *b, size_t n) {
  fbt t = {b, n, 0};
  if (n >= 4) t.pos = le32(b);
  return t;
}
static uint64_t fb_u64(const fbt *t, uint16_t vto) {
  uint16_t o = fb_offset(t, vto);
  if (o && fb_ok(t, (uint64_t)t->pos + o, 8)) return le64(t->b + t->pos + o);
  return 0;
}

/* generated accessors (pkg/tempofb/{SearchEntry,SearchPage,SearchBlockHeader,KeyValues}.go): SearchEntry{id 4, tags 6, start 8, end 10},
 * SearchPage{tags 4, entries 6}, SearchBlockHeader{tags 4, min 6, max 8}, KeyValues{key 4, value 6}.
 * A "tag container" (FBTagContainer, searchdata_util.go:42-45) is any table whose
 * [KeyValues] vector sits at vtable offset tag_vto. */
#define VT_ENTRY_ID 4
#define VT_ENTRY_TAGS 6
#define VT_ENTRY_START 8
#define VT_ENTRY_END 10
#define VT_PAGE_TAGS 4
#define VT_PAGE_ENTRIES 6
#define VT_HDR_TAGS 4
#define VT_HDR_MIN 6
#define VT_HDR_MAX 8
#define VT_KV_KEY 4
#define VT_KV_VALUE 6

static uint32_t tc_len(const fbt *t, uint16_t tag_vto) { /* TagsLength */
  uint16_t o = fb_offset(t, tag_vto);
  return o ? fb_vector_len(t, o) : 0;
}
static int tc_tag(const fbt *t, uint16_t tag_vto, uint32_t j, fbt *kv) { /* Tags(obj, j) */
  uint16_t o = fb_offset(t, tag_vto);
  if (!o) return 0;
  uint32_t x = fb_vector(t, o) + j * 4;
  kv->b = t->b;
  kv->n = t->n;
  kv->pos = fb_indirect(t, x);
  return 1;
}
static const uint8_t *kv_key(const fbt *kv, uint32_t *len) { /* KeyValues.Key */
  uint16_t o = fb_offset(kv, VT_KV_KEY);
  if (!o) { *len = 0; return NULL; }
  return fb_byte_vector(kv, o + kv->pos, len);
}
static uint32_t kv_value_len(const fbt *kv) {
  uint16_t o = fb_offset(kv, VT_KV_VALUE);
  return o ? fb_vector_len(kv, o) : 0;
}
static const uint8_t *kv_value(const fbt *kv, uint32_t j, uint32_t *len) { /* KeyValues.Value(j) */
  uint16_t o = fb_offset(kv, VT_KV_VALUE);
  if (!o) { *len = 0; return NULL; }
  uint32_t a = fb_vector(kv, o);
  return fb_byte_vector(kv, a + j * 4, len);
}

/* FindTag / binarySearch (pkg/tempofb/searchdata_util.go:63-100): the vector is
 * written descending, so the comparator is bytes.Compare(kv.Key(), k) and
 * cmp=-1 -> j=h, +1 -> i=h+1. */
static int find_tag(const fbt *t, uint16_t tag_vto, const uint8_t *k, size_t kl, fbt *kv) {
  uint32_t i = 0, j = tc_len(t, tag_vto);
  while (i < j) {
    uint32_t h = (i + j) >> 1;
    tc_tag(t, tag_vto, h, kv);
    uint32_t klen;
    const uint8_t *key = kv_key(kv, &klen);
    int c = bytes_compare(key, klen, k, kl);
    if (c == 0) return 1;
    if (c == -1) j = h;
    else i = h + 1;
  }
  return 0;
}
/* ContainsTag (searchdata_util.go:47-61) */
static int contains_tag(const fbt *t, uint16_t tag_vto, const uint8_t *k, size_t kl, const uint8_t *v,
                        size_t vl) {
  fbt kv;
  if (!find_tag(t, tag_vto, k, kl, &kv)) return 0;
  uint32_t l = kv_value_len(&kv);
  for (uint32_t j = 0; j < l; j++) {
    uint32_t len;
    const uint8_t *val = kv_value(&kv, j, &len);
    if (bytes_contains(val, len, v, vl)) return 1;
  }
  return 0;
}
/* SearchEntry.Get (searchdata_util.go:10-23): linear scan, Value(0) of first key match. */
static const uint8_t *entry_get(const fbt *e, const char *k, uint32_t *len) {
  size_t kl = strlen(k);
  uint32_t n = tc_len(e, VT_ENTRY_TAGS);
  fbt kv;
  for (uint32_t i = 0; i < n; i++) {
    tc_tag(e, VT_ENTRY_TAGS, i, &kv);
    uint32_t klen;
    const uint8_t *key = kv_key(&kv, &klen);
    if (klen == kl && memcmp(key, k, kl) == 0) {
      if (kv_value_len(&kv) == 0) { *len = 0; return NULL; }
      return kv_value(&kv, 0, len);
    }
  }
  *len = 0;
  return NULL;
}

/* ------------------------------------------------------------------------- */
/* strings.ToLower (Go). ASCII exactly; beyond ASCII a documented subset of
 * unicode.ToLower (Latin-1, Latin Extended-A, Greek, Cyrillic, Armenian) and
 * invalid UTF-8 -> U+FFFD as strings.Map does. Non-ASCII folding is
 * "parity unpinned" (DESIGN.md): the Go host passes lowered bytes (pitfall P4). */
static uint32_t uni_lower(uint32_t r) {
  if (r >= 'A' && r <= 'Z') return r + 32;
  if (r < 0x80) return r;
  if (r >= 0xC0 && r <= 0xDE && r != 0xD7) return r + 32;
  if (r == 0x130) return 0x69;
  if (r == 0x178) return 0xFF;
  if ((r >= 0x100 && r <= 0x12F) || (r >= 0x132 && r <= 0x137) || (r >= 0x14A && r <= 0x177))
    return (r & 1) ? r : r + 1;
  if ((r >= 0x139 && r <= 0x148) || (r >= 0x179 && r <= 0x17E)) return (r & 1) ? r + 1 : r;
  if (r == 0x386) return 0x3AC;
  if (r >= 0x388 && r <= 0x38A) return r + 37;
  if (r == 0x38C) return 0x3CC;
  if (r == 0x38E || r == 0x38F) return r + 63;
  if ((r >= 0x391 && r <= 0x3A1) || (r >= 0x3A3 && r <= 0x3AB)) return r + 32;
  if (r >= 0x400 && r <= 0x40F) return r + 80;
  if (r >= 0x410 && r <= 0x42F) return r + 32;
  if (r >= 0x531 && r <= 0x556) return r + 48;
  return r;
}
/* utf8.DecodeRune: returns rune and width; invalid -> (0xFFFD, 1) */
static uint32_t utf8_decode(const uint8_t *s, size_t n, size_t *w) {
  uint8_t c = s[0];
  if (c < 0x80) { *w = 1; return c; }
  uint32_t r;
  size_t need;
  uint32_t minv;
  if (c >= 0xC2 && c <= 0xDF) { need = 2; r = c & 0x1F; minv = 0x80; }
  else if (c >= 0xE0 && c <= 0xEF) { need = 3; r = c & 0x0F; minv = 0x800; }
  else if (c >= 0xF0 && c <= 0xF4) { need = 4; r = c & 0x07; minv = 0x10000; }
  else { *w = 1; return 0xFFFD; }
  if (n < need) { *w = 1; return 0xFFFD; }
  for (size_t i = 1; i < need; i++) {
    if ((s[i] & 0xC0) != 0x80) { *w = 1; return 0xFFFD; }
    r = (r << 6) | (s[i] & 0x3F);
  }
  if (r < minv || r > 0x10FFFF || (r >= 0xD800 && r <= 0xDFFF)) { *w = 1; return 0xFFFD; }
  *w = need;
  return r;
}
static size_t utf8_encode(uint32_t r, uint8_t *o) {
  if (r < 0x80) { o[0] = (uint8_t)r; return 1; }
  if (r < 0x800) { o[0] = 0xC0 | (r >> 6); o[1] = 0x80 | (r & 0x3F); return 2; }
  if (r < 0x10000) { o[0] = 0xE0 | (r >> 12); o[1] = 0x80 | ((r >> 6) & 0x3F); o[2] = 0x80 | (r & 0x3F); return 3; }
  o[0] = 0xF0 | (r >> 18); o[1] = 0x80 | ((r >> 12) & 0x3F); o[2] = 0x80 | ((r >> 6) & 0x3F); o[3] = 0x80 | (r & 0x3F);
  return 4;
}
/* out must hold 3*n bytes */
static size_t go_to_lower(const uint8_t *s, size_t n, uint8_t *out) {
  int ascii = 1;
  for (size_t i = 0; i < n; i++)
    if (s[i] >= 0x80) { ascii = 0; break; }
  if (ascii) {
    for (size_t i = 0; i < n; i++) out[i] = (s[i] >= 'A' && s[i] <= 'Z') ? s[i] + 32 : s[i];
    return n;
  }
  size_t o = 0;
  for (size_t i = 0; i < n;) {
    size_t w;
    uint32_t r = utf8_decode(s + i, n - i, &w);
    o += utf8_encode(uni_lower(r), out + o);
    i += w;
  }
  return o;
}

/* ------------------------------------------------------------------------- */
/* Pipeline (tempodb/search/pipeline.go:26-183)                                  */
typedef struct orc_pipeline {
  uint32_t nterms;
  uint8_t **k, **v;
  size_t *kl, *vl;
  int has_min, has_max, has_range, exhaustive;
  uint64_t min_ns, max_ns;
  uint32_t start, end;
} orc_pipeline;

static int eqs(const uint8_t *a, size_t al, const char *s) { return al == strlen(s) && memcmp(a, s, al) == 0; }

/* NewSearchPipeline + rewriteTagLookup (pipeline.go:26-140) */
static void pipeline_new(const orc_request *req, orc_pipeline *p) {
  memset(p, 0, sizeof(*p));
  if (req->min_duration_ms > 0) {
    p->has_min = 1;
    p->min_ns = (uint64_t)req->min_duration_ms * 1000000ULL;
  }
  if (req->max_duration_ms > 0) {
    p->has_max = 1;
    p->max_ns = (uint64_t)req->max_duration_ms * 1000000ULL;
  }
  if (req->start != 0 && req->end != 0) {
    p->has_range = 1;
    p->start = req->start;
    p->end = req->end;
  }
  p->k = (uint8_t **)calloc(req->ntags + 1, sizeof(uint8_t *));
  p->v = (uint8_t **)calloc(req->ntags + 1, sizeof(uint8_t *));
  p->kl = (size_t *)calloc(req->ntags + 1, sizeof(size_t));
  p->vl = (size_t *)calloc(req->ntags + 1, sizeof(size_t));
  for (uint32_t i = 0; i < req->ntags; i++) {
    const uint8_t *k = req->tag_keys[i], *v = req->tag_values[i];
    size_t kl = req->tag_key_lens[i], vl = req->tag_value_lens[i];
    const char *nk = NULL, *nv = NULL;
    if (eqs(k, kl, "x-dbg-exhaustive")) { /* SecretExhaustiveSearchTag */
      p->exhaustive = 1;
      continue;
    } else if (eqs(k, kl, "error")) { /* trace.ErrorTag */
      if (eqs(v, vl, "true")) { nk = "status.code"; nv = "2"; }
    } else if (eqs(k, kl, "status.code")) { /* StatusCodeMapping (pkg/model/trace/matches.go:27-31) */
      if (eqs(v, vl, "unset")) { nk = "status.code"; nv = "0"; }
      else if (eqs(v, vl, "ok")) { nk = "status.code"; nv = "1"; }
      else if (eqs(v, vl, "error")) { nk = "status.code"; nv = "2"; }
    }
    if (nk) { k = (const uint8_t *)nk; kl = strlen(nk); v = (const uint8_t *)nv; vl = strlen(nv); }
    uint32_t t = p->nterms++;
    p->k[t] = (uint8_t *)malloc(3 * kl + 1);
    p->v[t] = (uint8_t *)malloc(3 * vl + 1);
    p->kl[t] = go_to_lower(k, kl, p->k[t]);
    p->vl[t] = go_to_lower(v, vl, p->v[t]);
  }
}
static void pipeline_free(orc_pipeline *p) {
  for (uint32_t i = 0; i < p->nterms; i++) { free(p->k[i]); free(p->v[i]); }
  free(p->k); free(p->v); free(p->kl); free(p->vl);
}
static int tagfilter(const orc_pipeline *p, const fbt *t, uint16_t vto) {
  for (uint32_t i = 0; i < p->nterms; i++)
    if (!contains_tag(t, vto, p->k[i], p->kl[i], p->v[i], p->vl[i])) return 0;
  return 1;
}
/* Pipeline.Matches: trace filters then tag filter (pipeline.go:142-157) */
static int pipeline_matches(const orc_pipeline *p, const fbt *e) {
  uint64_t st = fb_u64(e, VT_ENTRY_START), et = fb_u64(e, VT_ENTRY_END);
  if (p->has_min && !((et - st) >= p->min_ns)) return 0;
  if (p->has_max && !((et - st) <= p->max_ns)) return 0;
  if (p->has_range) {
    uint32_t ss = (uint32_t)(st / 1000000000ULL), es = (uint32_t)(et / 1000000000ULL);
    if (!(p->start <= es && p->end >= ss)) return 0;
  }
  if (p->exhaustive) return 0;
  return tagfilter(p, e, VT_ENTRY_TAGS);
}
/* MatchesBlock (pipeline.go:172-183), blockfilters built at :38-41 and :53-56 */
static int pipeline_matches_block(const orc_pipeline *p, const fbt *h) {
  if (p->has_min && !(fb_u64(h, VT_HDR_MAX) >= p->min_ns)) return 0;
  if (p->has_max && !(fb_u64(h, VT_HDR_MIN) <= p->max_ns)) return 0;
  return tagfilter(p, h, VT_HDR_TAGS);
}

int orc_pipeline_matches_entry(const orc_request *req, const uint8_t *fb, size_t len) {
  orc_pipeline p;
  pipeline_new(req, &p);
  fbt e = fb_root(fb, len);
  int m = pipeline_matches(&p, &e);
  pipeline_free(&p);
  return m;
}
int orc_pipeline_matches_block(const orc_request *req, const uint8_t *fb, size_t len) {
  orc_pipeline p;
  pipeline_new(req, &p);
  fbt h = fb_root(fb, len);
  int m = pipeline_matches_block(&p, &h);
  pipeline_free(&p);
  return m;
}
int orc_contains_tag_entry(const uint8_t *fb, size_t len, const uint8_t *k, size_t kl, const uint8_t *v,
                           size_t vl) {
  fbt e = fb_root(fb, len);
  return contains_tag(&e, VT_ENTRY_TAGS, k, kl, v, vl);
}

/* ------------------------------------------------------------------------- */
/* files                                                                       */
static int read_file(const char *dir, const char *name, uint8_t **out, size_t *len) {
  char path[4096];
  snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE *f = fopen(path, "rb");
  if (!f) return errno == ENOENT ? ORC_NOT_FOUND : ORC_IO;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *b = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
  if (n > 0 && fread(b, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(b); return ORC_IO; }
  fclose(f);
  *out = b;
  *len = (size_t)n;
  return ORC_OK;
}

/* minimal JSON field readers for the meta files */
static const char *json_field(const char *js, size_t n, const char *name) {
  char pat[128];
  snprintf(pat, sizeof pat, "\"%s\"", name);
  const char *p = (const char *)memmem(js, n, pat, strlen(pat));
  if (!p) return NULL;
  p += strlen(pat);
  while (*p == ' ' || *p == ':') p++;
  return p;
}
static int json_u64(const char *js, size_t n, const char *name, uint64_t *v) {
  const char *p = json_field(js, n, name);
  if (!p) return 0;
  *v = strtoull(p, NULL, 10);
  return 1;
}
static int json_str(const char *js, size_t n, const char *name, char *out, size_t cap) {
  const char *p = json_field(js, n, name);
  if (!p || *p != '"') return 0;
  p++;
  size_t i = 0;
  while (*p && *p != '"' && i + 1 < cap) out[i++] = *p++;
  out[i] = 0;
  return 1;
}
/* backend.ParseEncoding (tempodb/backend/encoding.go:104-112), case-insensitive */
static int parse_encoding(const char *s) {
  static const char *names[] = {"none", "gzip", "lz4-64k", "lz4-256k", "lz4-1M", "lz4", "snappy", "zstd", "s2"};
  for (int i = 0; i < 9; i++)
    if (strcasecmp(s, names[i]) == 0) return i;
  return -1;
}

/* ------------------------------------------------------------------------- */
/* v2 framing                                                                  */
/* unmarshalPageFromBytes (tempodb/encoding/v2/page.go:30-57) */
static int unmarshal_page(const uint8_t *b, size_t n, size_t hdr_len_expected, const uint8_t **hdr,
                          const uint8_t **data, size_t *dlen) {
  size_t total_hdr = 6 + hdr_len_expected;
  if (n < total_hdr) return ORC_CORRUPT;
  uint32_t total = le32(b);
  uint16_t hl = le16(b + 4);
  if ((size_t)hl > n - 6) return ORC_CORRUPT;
  if (hl != hdr_len_expected) return ORC_CORRUPT; /* dataHeader/indexHeader.unmarshalHeader */
  *hdr = b + 6;
  const uint8_t *rest = b + 6 + hl;
  size_t rl = n - 6 - hl;
  int64_t dl = (int64_t)total - (int64_t)total_hdr;
  if (dl < 0 || (size_t)dl != rl) return ORC_CORRUPT;
  *data = rest;
  *dlen = rl;
  return ORC_OK;
}

/* search-index / index reader (tempodb/encoding/v2/index_reader.go) */
typedef struct orc_index {
  const uint8_t *buf;
  size_t len;
  uint32_t page_size, total;
  uint32_t per_page;
  /* verified pages cache (pageCache) */
  int8_t *checked;
  size_t npages;
} orc_index;
static void index_init(orc_index *ix, const uint8_t *buf, size_t len, uint32_t page_size, uint32_t total) {
  ix->buf = buf;
  ix->len = len;
  ix->page_size = page_size;
  ix->total = total;
  /* objectsPerPage(28, pageSize, 8) (page.go:175-182) */
  ix->per_page = page_size > 14 ? (page_size - 8 - 6) / 28 : 0;
  ix->npages = page_size ? (len + page_size - 1) / page_size : 0;
  ix->checked = (int8_t *)calloc(ix->npages + 1, 1);
}
static void index_free(orc_index *ix) { free(ix->checked); }
/* getPage (index_reader.go:116-143): read pageSize bytes at pageIdx*pageSize,
 * unmarshal with an 8-byte header, verify xxhash64 of the page data. */
static int index_page(orc_index *ix, size_t pidx, const uint8_t **data, size_t *dlen) {
  uint64_t off = (uint64_t)pidx * ix->page_size;
  if (off + ix->page_size > ix->len) return ORC_CORRUPT; /* ReadAt short read */
  const uint8_t *hdr;
  int rc = unmarshal_page(ix->buf + off, ix->page_size, 8, &hdr, data, dlen);
  if (rc) return rc;
  if (!ix->checked[pidx]) {
    if (le64(hdr) != orc_xxhash64(*data, *dlen)) return ORC_CORRUPT; /* mismatched checksum */
    ix->checked[pidx] = 1;
  }
  return ORC_OK;
}
/* At (index_reader.go:42-82); returns 1 record, 0 past end, <0 error */
static int index_at(orc_index *ix, int64_t i, const uint8_t **rec) {
  if (i < 0 || i >= (int64_t)ix->total) return 0;
  if (ix->per_page == 0) return -ORC_CORRUPT;
  size_t pidx = (size_t)(i / ix->per_page), ridx = (size_t)(i % ix->per_page);
  const uint8_t *data;
  size_t dlen;
  int rc = index_page(ix, pidx, &data, &dlen);
  if (rc) return -rc;
  if (ridx >= dlen / 28) return -ORC_CORRUPT;
  const uint8_t *r = data + ridx * 28;
  int zero = 1;
  for (int k = 0; k < 28; k++)
    if (r[k]) { zero = 0; break; }
  if (zero) return -ORC_CORRUPT;
  *rec = r;
  return 1;
}
/* Find (index_reader.go:85-114) with sort.SearchWithErrors (pkg/sort/search.go:5-24) */
static int index_find(orc_index *ix, const uint8_t *id, size_t idl, int64_t *out) {
  int64_t i = 0, j = ix->total;
  while (i < j) {
    int64_t h = (int64_t)(((uint64_t)(i + j)) >> 1);
    const uint8_t *r;
    int rc = index_at(ix, h, &r);
    if (rc < 0) return -rc;
    if (!(bytes_compare(r, 16, id, idl) >= 0)) i = h + 1;
    else j = h;
  }
  *out = (i >= 0 && i < (int64_t)ix->total) ? i : -1;
  return ORC_OK;
}

/* dataReader.Read for one record + decompression (data_reader.go:45-125) */
static int data_read_page(const uint8_t *data, size_t dlen, int enc, uint64_t start, uint32_t length,
                          uint8_t **out, size_t *out_len) {
  if (start + length > dlen) return ORC_CORRUPT;
  const uint8_t *hdr, *payload;
  size_t pl;
  int rc = unmarshal_page(data + start, length, 0, &hdr, &payload, &pl);
  if (rc) return rc;
  if (enc == 0) { /* EncNone: pass-through reader */
    *out = (uint8_t *)malloc(pl ? pl : 1);
    memcpy(*out, payload, pl);
    *out_len = pl;
    return ORC_OK;
  }
  if (enc == 6) return orc_snappy_framed_decode(payload, pl, out, out_len);
  return ORC_UNSUPPORTED_ENCODING;
}

/* object.UnmarshalAndAdvanceBuffer (object.go:82-113) */
static int unmarshal_advance(const uint8_t **buf, size_t *len, const uint8_t **id, uint32_t *idl,
                             const uint8_t **obj, size_t *objl) {
  if (*len == 0) return 1; /* io.EOF */
  if (*len < 4) return -ORC_CORRUPT;
  uint32_t total = le32(*buf);
  if (*len - 4 < 4) return -ORC_CORRUPT;
  uint32_t il = le32(*buf + 4);
  const uint8_t *b = *buf + 8;
  size_t bl = *len - 8;
  uint32_t rest = total - 8;
  if ((uint64_t)bl < rest) return -ORC_CORRUPT;
  if (il > rest) return -ORC_CORRUPT; /* Go would panic on the slice */
  *id = b;
  *idl = il;
  *obj = b + il;
  *objl = rest - il;
  *buf = b + rest;
  *len = bl - rest;
  return 0;
}

/* object.UnmarshalObjectFromReader (object.go:50-80) over a bytes.Reader holding buf[0 .. len):
 * what findOne's iterator calls (iterator.go:30-32, finder_paged.go:89). Not the function above:
 * the page's end differs. binary.Read is io.ReadFull of 4 bytes (encoding/binary, io.ReadAtLeast):
 * io.EOF with nothing left, io.ErrUnexpectedEOF with 1..3 left. The id and object are one
 * r.Read(b), len(b) = total - 8 as a uint32: bytes.Reader.Read answers io.EOF whenever the reader
 * is at its end (also for an empty b), else copies what is left without an error, and a short
 * count is the "read %d but expected %d" error (:69-71). Returns 1 for io.EOF (the iterator's
 * clean end), < 0 for any other error. */
static int unmarshal_from_reader(const uint8_t **buf, size_t *len, const uint8_t **id, uint32_t *idl,
                                 const uint8_t **obj, size_t *objl) {
  for (int field = 0; field < 2; field++) { /* totalLength (:52), idLength (:58) */
    const size_t left = *len - 4u * (size_t)field;
    if (left == 0) return 1;
    if (left < 4) return -ORC_CORRUPT;
  }
  const uint32_t total = le32(*buf), il = le32(*buf + 4);
  const uint8_t *b = *buf + 8;
  const size_t bl = *len - 8;
  const uint32_t rest = total - 8; /* (:63, wraps below 8 as the uint32 does) */
  if (bl == 0) return 1;           /* r.Read at the reader's end (:65-68) */
  if ((uint64_t)bl < rest) return -ORC_CORRUPT; /* short read (:69-71) */
  if (il > rest) return -ORC_CORRUPT;           /* id length outside the buffer (:72-74) */
  *id = b;
  *idl = il;
  *obj = b + il;
  *objl = rest - il;
  *buf = b + rest;
  *len = bl - rest;
  return 0;
}

/* ------------------------------------------------------------------------- */
/* backend search block                                                        */
struct orc_block {
  int wal; /* a search WAL file (StreamingSearchBlock): data = the file, enc from its name */
  int live; /* live traces (instance.searchLiveTraces): data = segment bytes, seg_off/trace_seg */
  uint32_t ntraces;
  uint64_t nsegs;
  uint64_t *seg_off;   /* nsegs + 1 offsets into data */
  uint64_t *trace_seg; /* ntraces + 1: first segment of each trace */
  int has_meta;
  int enc;
  char version[16];
  uint32_t index_page_size, index_records;
  uint8_t *header;
  size_t header_len;
  uint8_t *index;
  size_t index_len;
  uint8_t *data;
  size_t data_len;
  /* a page range of the block (tempo_amd.shard's split of a large block over ranks):
   * index records [first_page, first_page + npages), npages 0 = to the end. A range that does
   * not start at page 0 counts neither the header's bytes nor the block as inspected/skipped
   * (the range at page 0 does), so the ranges' metrics sum to the whole block's. */
  uint32_t first_page, npages;
};

void orc_block_set_pages(orc_block *b, uint32_t first_page, uint32_t npages) {
  b->first_page = first_page;
  b->npages = npages;
}

int orc_block_load(const char *dir, orc_block **out) {
  orc_block *b = (orc_block *)calloc(1, sizeof(*b));
  uint8_t *meta;
  size_t ml;
  int rc = read_file(dir, "search.meta.json", &meta, &ml);
  if (rc == ORC_NOT_FOUND) { *out = b; return ORC_OK; } /* Search is a no-op */
  if (rc) { free(b); return rc; }
  b->has_meta = 1;
  char enc[32] = {0};
  uint64_t v;
  json_str((const char *)meta, ml, "version", b->version, sizeof b->version);
  json_str((const char *)meta, ml, "encoding", enc, sizeof enc);
  b->enc = parse_encoding(enc);
  b->index_page_size = json_u64((const char *)meta, ml, "indexPageSize", &v) ? (uint32_t)v : 0;
  b->index_records = json_u64((const char *)meta, ml, "indexRecords", &v) ? (uint32_t)v : 0;
  free(meta);
  if ((rc = read_file(dir, "search-header", &b->header, &b->header_len)) ||
      (rc = read_file(dir, "search-index", &b->index, &b->index_len)) ||
      (rc = read_file(dir, "search", &b->data, &b->data_len))) {
    orc_block_free(b);
    return rc;
  }
  *out = b;
  return ORC_OK;
}
void orc_block_free(orc_block *b) {
  if (!b) return;
  free(b->seg_off);
  free(b->trace_seg);
  free(b->header);
  free(b->index);
  free(b->data);
  free(b);
}
uint64_t orc_block_bytes(const orc_block *b) { return b->header_len + b->index_len + b->data_len; }

/* growable match list */
typedef struct mlist {
  orc_match *m;
  uint64_t n, cap;
  char *s;
  uint64_t sl, scap;
  orc_metrics met;
  int status;
  int32_t *bstat; /* per block (orc_search) */
  uint64_t nb;
} mlist;
static uint32_t ml_str(mlist *l, const uint8_t *p, uint32_t n) {
  if (l->sl + n + 1 > l->scap) {
    while (l->sl + n + 1 > l->scap) l->scap = l->scap ? l->scap * 2 : 4096;
    l->s = (char *)realloc(l->s, l->scap);
  }
  uint32_t off = (uint32_t)l->sl;
  if (n) memcpy(l->s + l->sl, p, n);
  l->s[l->sl + n] = 0;
  l->sl += n + 1;
  return off;
}
static orc_match *ml_push(mlist *l) {
  if (l->n == l->cap) {
    l->cap = l->cap ? l->cap * 2 : 256;
    l->m = (orc_match *)realloc(l->m, l->cap * sizeof(orc_match));
  }
  return &l->m[l->n++];
}

/* consumer state: deterministic refinement of instance.Search's loop
 * (modules/ingester/instance_search.go:45-60): stop right after the first
 * occurrence of the limit-th distinct trace ID. */
/* Trace IDs are keyed by their right-aligned 16 bytes: TraceIDToHexString trims
 * leading zeros, so hex-string equality == right-aligned byte equality. */
typedef struct idset {
  uint8_t (*k)[16];
  uint8_t *used;
  uint64_t cap, n;
} idset;
static int idset_add(idset *s, const uint8_t *id16) { /* 1 if new */
  if (s->n * 2 + 2 > s->cap) {
    uint64_t nc = s->cap ? s->cap * 2 : 64;
    uint8_t(*nk)[16] = (uint8_t(*)[16])calloc(nc, 16);
    uint8_t *nu = (uint8_t *)calloc(nc, 1);
    for (uint64_t i = 0; i < s->cap; i++) {
      if (!s->used[i]) continue;
      uint64_t h = orc_xxhash64(s->k[i], 16) & (nc - 1);
      while (nu[h]) h = (h + 1) & (nc - 1);
      memcpy(nk[h], s->k[i], 16);
      nu[h] = 1;
    }
    free(s->k);
    free(s->used);
    s->k = nk;
    s->used = nu;
    s->cap = nc;
  }
  uint64_t h = orc_xxhash64(id16, 16) & (s->cap - 1);
  while (s->used[h]) {
    if (memcmp(s->k[h], id16, 16) == 0) return 0;
    h = (h + 1) & (s->cap - 1);
  }
  memcpy(s->k[h], id16, 16);
  s->used[h] = 1;
  s->n++;
  return 1;
}

/* GetSearchResultFromData (tempodb/search/util.go:27-35) for entry e -> m */
static int result_from_entry(const fbt *e, uint32_t bidx, uint64_t scan_pos, mlist *out, orc_match **mo) {
  orc_match *m = ml_push(out);
  memset(m, 0, sizeof *m);
  uint32_t il = 0;
  const uint8_t *tid = NULL;
  uint16_t io = fb_offset(e, VT_ENTRY_ID);
  if (io) tid = fb_byte_vector(e, io + e->pos, &il);
  if (il > 16) return ORC_CORRUPT;
  if (il) memcpy(m->id + 16 - il, tid, il);
  m->id_len = il;
  m->block_idx = bidx;
  m->entry_idx = scan_pos;
  m->start_ns = fb_u64(e, VT_ENTRY_START);
  m->end_ns = fb_u64(e, VT_ENTRY_END);
  m->duration_ms = (uint32_t)((m->end_ns - m->start_ns) / 1000000ULL);
  uint32_t sl, nl;
  const uint8_t *sv = entry_get(e, "root.service.name", &sl);
  const uint8_t *nv = entry_get(e, "root.name", &nl);
  m->svc_off = ml_str(out, sv, sl);
  m->svc_len = sl;
  m->name_off = ml_str(out, nv, nl);
  m->name_len = nl;
  *mo = m;
  return ORC_OK;
}

/* BackendSearchBlock.Search (tempodb/search/backend_search_block.go:184-298).
 * `stop` (optional) = consumer: called per match, returns 1 when the consumer
 * closed (the L-th distinct id arrived) -> the block stops right there. */
typedef int (*consume_fn)(void *ctx, const orc_match *m);
static int wal_search(const orc_block *b, uint32_t bidx, const orc_pipeline *p, mlist *out, consume_fn consume,
                      void *cctx, int *quit);
static int live_search(const orc_block *b, uint32_t bidx, const orc_pipeline *p, mlist *out, consume_fn consume,
                       void *cctx, int *quit);
static int block_search(const orc_block *b, uint32_t bidx, const orc_pipeline *p, mlist *out,
                        consume_fn consume, void *cctx, int *quit) {
  if (b->live) return live_search(b, bidx, p, out, consume, cctx, quit);
  if (b->wal) return wal_search(b, bidx, p, out, consume, cctx, quit);
  if (!b->has_meta) return ORC_OK; /* ErrDoesNotExist -> nil (:191-203) */
  if (strcmp(b->version, "v2") != 0) return ORC_UNSUPPORTED_ENCODING; /* encoding.FromVersion */
  const int tail = b->first_page > 0; /* a page range after the block's first page */
  if (!tail) out->met.bytes_inspected += b->header_len; /* :217 */
  fbt h = fb_root(b->header, b->header_len);
  if (!pipeline_matches_block(p, &h)) {
    if (!tail) out->met.blocks_skipped++;
    return ORC_OK;
  }
  if (!tail) out->met.blocks_inspected++;
  if (b->enc < 0) return ORC_UNSUPPORTED_ENCODING; /* NewDataReader -> getReaderPool */
  orc_index ix;
  index_init(&ix, b->index, b->index_len, b->index_page_size, b->index_records);
  int rc = ORC_OK;
  uint64_t scan_pos = 0; /* (a page range: positions inside the range) */
  const int64_t i_end = b->npages ? (int64_t)b->first_page + b->npages : INT64_MAX;
  for (int64_t i = b->first_page; i < i_end; i++) { /* for !sr.Quit() (:247) */
    if (*quit) break;
    const uint8_t *rec;
    int r = index_at(&ix, i, &rec);
    if (r <= 0) break; /* record == nil -> return nil (error is dropped: `record, _ := ir.At`) */
    uint64_t start = le64(rec + 16);
    uint32_t length = le32(rec + 24);
    uint8_t *page;
    size_t pl;
    rc = data_read_page(b->data, b->data_len, b->enc, start, length, &page, &pl);
    if (rc) break;
    const uint8_t *cur = page, *id, *obj;
    size_t cl = pl, objl;
    uint32_t idl;
    int u = unmarshal_advance(&cur, &cl, &id, &idl, &obj, &objl);
    if (u != 0) { rc = u < 0 ? -u : ORC_CORRUPT; free(page); break; }
    out->met.bytes_inspected += objl; /* :267 */
    fbt pg = fb_root(obj, objl);
    uint32_t ne = 0;
    uint16_t eo = fb_offset(&pg, VT_PAGE_ENTRIES);
    if (eo) ne = fb_vector_len(&pg, eo);
    if (!tagfilter(p, &pg, VT_PAGE_TAGS)) { /* MatchesPage (:271-276) */
      out->met.traces_inspected += ne;
      scan_pos += ne;
      free(page);
      continue;
    }
    for (uint32_t j = 0; j < ne; j++) {
      out->met.traces_inspected += 1;
      fbt e;
      e.b = pg.b;
      e.n = pg.n;
      e.pos = fb_indirect(&pg, fb_vector(&pg, eo) + j * 4);
      if (!pipeline_matches(p, &e)) { scan_pos++; continue; }
      /* GetSearchResultFromData (tempodb/search/util.go:27-35) */
      orc_match *m = ml_push(out);
      memset(m, 0, sizeof *m);
      uint32_t il = 0;
      const uint8_t *tid = NULL;
      uint16_t io = fb_offset(&e, VT_ENTRY_ID);
      if (io) tid = fb_byte_vector(&e, io + e.pos, &il);
      if (il > 16) { rc = ORC_CORRUPT; break; }
      memcpy(m->id + 16 - il, tid, il);
      m->id_len = il;
      m->block_idx = bidx;
      m->entry_idx = scan_pos;
      m->start_ns = fb_u64(&e, VT_ENTRY_START);
      m->end_ns = fb_u64(&e, VT_ENTRY_END);
      m->duration_ms = (uint32_t)((m->end_ns - m->start_ns) / 1000000ULL);
      uint32_t sl, nl;
      const uint8_t *sv = entry_get(&e, "root.service.name", &sl);
      const uint8_t *nv = entry_get(&e, "root.name", &nl);
      m->svc_off = ml_str(out, sv, sl);
      m->svc_len = sl;
      m->name_off = ml_str(out, nv, nl);
      m->name_len = nl;
      scan_pos++;
      if (consume && consume(cctx, m)) { *quit = 1; break; }
    }
    free(page);
    if (rc || *quit) break;
  }
  index_free(&ix);
  return rc;
}

typedef struct limit_ctx {
  idset ids;
  uint32_t limit;
  uint64_t distinct;
} limit_ctx;
static int limit_consume(void *c, const orc_match *m) {
  limit_ctx *lc = (limit_ctx *)c;
  if (idset_add(&lc->ids, m->id)) lc->distinct++;
  return lc->distinct >= lc->limit;
}

typedef struct thr_arg {
  const orc_block *b;
  uint32_t bidx;
  const orc_pipeline *p;
  mlist out;
  int rc;
} thr_arg;
static void *thr_main(void *a) {
  thr_arg *t = (thr_arg *)a;
  int quit = 0;
  t->rc = block_search(t->b, t->bidx, t->p, &t->out, NULL, NULL, &quit);
  return NULL;
}

static void finish(mlist *l, orc_result **out) {
  orc_result *r = (orc_result *)calloc(1, sizeof *r);
  r->n = l->n;
  r->m = l->m;
  r->strings = l->s;
  r->strings_len = l->sl;
  r->metrics = l->met;
  r->status = l->status;
  r->nblocks = l->nb;
  r->block_status = l->bstat;
  *out = r;
}

int orc_search_seeded(orc_block *const *blocks, uint32_t nblocks, const orc_request *req, uint32_t limit,
                      const uint8_t (*seen)[16], uint64_t nseen, orc_result **out);
int orc_search(orc_block *const *blocks, uint32_t nblocks, const orc_request *req, uint32_t limit,
               int nthreads, orc_result **out) {
  orc_pipeline p;
  pipeline_new(req, &p);
  mlist all;
  memset(&all, 0, sizeof all);
  all.nb = nblocks;
  all.bstat = (int32_t *)calloc(nblocks + 1, sizeof(int32_t));
  if (limit == 0 && nthreads > 1 && nblocks > 1) {
    /* one thread per block (instance.searchLocalBlocks: a goroutine per block),
     * at most nthreads in flight; concatenated in block order. */
    thr_arg *ta = (thr_arg *)calloc(nblocks, sizeof *ta);
    pthread_t *th = (pthread_t *)calloc(nblocks, sizeof *th);
    for (uint32_t base = 0; base < nblocks; base += (uint32_t)nthreads) {
      uint32_t e = base + (uint32_t)nthreads < nblocks ? base + (uint32_t)nthreads : nblocks;
      for (uint32_t i = base; i < e; i++) {
        ta[i].b = blocks[i];
        ta[i].bidx = i;
        ta[i].p = &p;
        pthread_create(&th[i], NULL, thr_main, &ta[i]);
      }
      for (uint32_t i = base; i < e; i++) pthread_join(th[i], NULL);
    }
    for (uint32_t i = 0; i < nblocks; i++) {
      mlist *l = &ta[i].out;
      for (uint64_t k = 0; k < l->n; k++) {
        orc_match *m = ml_push(&all);
        *m = l->m[k];
        m->svc_off = ml_str(&all, (const uint8_t *)l->s + l->m[k].svc_off, l->m[k].svc_len);
        m->name_off = ml_str(&all, (const uint8_t *)l->s + l->m[k].name_off, l->m[k].name_len);
      }
      all.met.traces_inspected += l->met.traces_inspected;
      all.met.blocks_inspected += l->met.blocks_inspected;
      all.met.blocks_skipped += l->met.blocks_skipped;
      all.met.bytes_inspected += l->met.bytes_inspected;
      if (ta[i].rc && !all.status) all.status = ta[i].rc;
      all.bstat[i] = ta[i].rc;
      free(l->m);
      free(l->s);
    }
    free(ta);
    free(th);
  } else {
    limit_ctx lc;
    memset(&lc, 0, sizeof lc);
    lc.limit = limit;
    int quit = 0;
    for (uint32_t i = 0; i < nblocks && !quit; i++) {
      int rc = block_search(blocks[i], i, &p, &all, limit ? limit_consume : NULL, &lc, &quit);
      if (rc && !all.status) all.status = rc; /* searchLocalBlocks logs and continues */
      all.bstat[i] = rc;
    }
    free(lc.ids.k);
    free(lc.ids.used);
  }
  pipeline_free(&p);
  finish(&all, out);
  return ORC_OK;
}

/* The sequential consumer of instance.Search (instance_search.go:45-60) whose id map already
 * holds `seen` (the distinct trace IDs a consumer took from blocks before these): it stops
 * where that consumer, having taken them first, would stop. The rank fan-out of a limit
 * search (tempo_amd/shard.py distributed_search_limit) is checked against it. */
int orc_search_seeded(orc_block *const *blocks, uint32_t nblocks, const orc_request *req, uint32_t limit,
                      const uint8_t (*seen)[16], uint64_t nseen, orc_result **out) {
  orc_pipeline p;
  pipeline_new(req, &p);
  mlist all;
  memset(&all, 0, sizeof all);
  all.nb = nblocks;
  all.bstat = (int32_t *)calloc(nblocks + 1, sizeof(int32_t));
  limit_ctx lc;
  memset(&lc, 0, sizeof lc);
  lc.limit = limit;
  for (uint64_t i = 0; i < nseen; i++)
    if (idset_add(&lc.ids, seen[i])) lc.distinct++;
  int quit = limit && lc.distinct >= limit;
  for (uint32_t i = 0; i < nblocks && !quit; i++) {
    int rc = block_search(blocks[i], i, &p, &all, limit ? limit_consume : NULL, &lc, &quit);
    if (rc && !all.status) all.status = rc;
    all.bstat[i] = rc;
  }
  free(lc.ids.k);
  free(lc.ids.used);
  pipeline_free(&p);
  finish(&all, out);
  return ORC_OK;
}

/* instance.Search consumer + CombineSearchResults + sort (instance_search.go:45-70,
 * tempodb/search/util.go:40-62). Deterministic: tie on start -> first position. */
typedef struct fin {
  orc_match m;
  uint64_t first;
} fin;
static int fin_cmp(const void *a, const void *b) {
  const fin *x = (const fin *)a, *y = (const fin *)b;
  if (x->m.start_ns != y->m.start_ns) return x->m.start_ns > y->m.start_ns ? -1 : 1;
  return x->first < y->first ? -1 : (x->first > y->first);
}
int orc_combine(const orc_result *in, uint32_t max_results, orc_result **out) {
  if (max_results == 0) max_results = 20;
  fin *f = (fin *)calloc(in->n + 1, sizeof *f);
  uint64_t nf = 0;
  for (uint64_t i = 0; i < in->n; i++) {
    const orc_match *m = &in->m[i];
    uint64_t j;
    for (j = 0; j < nf; j++) /* map lookup by TraceID (small lists) */
      if (memcmp(f[j].m.id, m->id, 16) == 0) break;
    if (j < nf) {
      orc_match *e = &f[j].m;
      if (e->svc_len == 0) { e->svc_off = m->svc_off; e->svc_len = m->svc_len; }
      if (e->name_len == 0) { e->name_off = m->name_off; e->name_len = m->name_len; }
      if (e->start_ns > m->start_ns) e->start_ns = m->start_ns;
      if (e->duration_ms < m->duration_ms) e->duration_ms = m->duration_ms;
    } else {
      f[nf].m = *m;
      f[nf].first = i;
      nf++;
    }
    if (nf >= max_results) break;
  }
  qsort(f, nf, sizeof *f, fin_cmp);
  orc_result *r = (orc_result *)calloc(1, sizeof *r);
  r->n = nf;
  r->m = (orc_match *)calloc(nf + 1, sizeof(orc_match));
  for (uint64_t i = 0; i < nf; i++) r->m[i] = f[i].m;
  r->strings = (char *)malloc(in->strings_len + 1);
  memcpy(r->strings, in->strings, in->strings_len);
  r->strings_len = in->strings_len;
  r->metrics = in->metrics;
  free(f);
  *out = r;
  return ORC_OK;
}
void orc_result_free(orc_result *r) {
  if (!r) return;
  free(r->m);
  free(r->strings);
  free(r->block_status);
  free(r);
}

/* ------------------------------------------------------------------------- */
/* v2 trace blocks: bloom + index + findOne                                    */
struct orc_v2block {
  uint8_t block_id[16];
  uint8_t min_id[64], max_id[64];
  size_t min_len, max_len;
  int64_t start_unix, end_unix;
  int enc;
  uint32_t index_page_size, total_records;
  uint32_t bloom_shards; /* meta value (0 -> legacy 10) */
  uint8_t **bloom;
  size_t *bloom_len;
  uint32_t nbloom;
  uint8_t *index;
  size_t index_len;
  uint8_t *data;
  size_t data_len;
};

static int b64val(char c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}
static size_t b64dec(const char *s, uint8_t *o, size_t cap) {
  size_t n = 0;
  uint32_t acc = 0;
  int bits = 0;
  for (; *s && *s != '"'; s++) {
    int v = b64val(*s);
    if (v < 0) continue;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      if (n < cap) o[n++] = (uint8_t)(acc >> bits);
    }
  }
  return n;
}
static int64_t days_from_civil(int64_t y, unsigned m, unsigned d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const unsigned yoe = (unsigned)(y - era * 400);
  const unsigned doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (int64_t)doe - 719468;
}
/* time.Time JSON (RFC3339Nano) -> Unix() seconds */
static int64_t rfc3339_unix(const char *s) {
  int Y, M, D, h, mi, se;
  if (sscanf(s, "%d-%d-%dT%d:%d:%d", &Y, &M, &D, &h, &mi, &se) != 6) return 0;
  const char *p = strchr(s, 'T');
  p += 9; /* hh:mm:ss */
  if (*p == '.')
    do p++; while (*p >= '0' && *p <= '9');
  int64_t off = 0;
  if (*p == '+' || *p == '-') {
    int oh = 0, om = 0;
    sscanf(p + 1, "%d:%d", &oh, &om);
    off = (oh * 3600 + om * 60) * (*p == '-' ? -1 : 1);
  }
  return days_from_civil(Y, (unsigned)M, (unsigned)D) * 86400 + h * 3600 + mi * 60 + se - off;
}
static void parse_uuid(const char *s, uint8_t out[16]) {
  int n = 0;
  for (; *s && *s != '"' && n < 32; s++) {
    int v;
    if (*s >= '0' && *s <= '9') v = *s - '0';
    else if (*s >= 'a' && *s <= 'f') v = *s - 'a' + 10;
    else if (*s >= 'A' && *s <= 'F') v = *s - 'A' + 10;
    else continue;
    if (n % 2 == 0) out[n / 2] = (uint8_t)(v << 4);
    else out[n / 2] |= (uint8_t)v;
    n++;
  }
}

int orc_v2block_load(const char *dir, orc_v2block **out) {
  uint8_t *meta;
  size_t ml;
  int rc = read_file(dir, "meta.json", &meta, &ml);
  if (rc) return rc;
  orc_v2block *b = (orc_v2block *)calloc(1, sizeof *b);
  const char *js = (const char *)meta;
  char enc[32] = {0};
  uint64_t v;
  json_str(js, ml, "encoding", enc, sizeof enc);
  b->enc = parse_encoding(enc);
  b->index_page_size = json_u64(js, ml, "indexPageSize", &v) ? (uint32_t)v : 0;
  b->total_records = json_u64(js, ml, "totalRecords", &v) ? (uint32_t)v : 0;
  b->bloom_shards = json_u64(js, ml, "bloomShards", &v) ? (uint32_t)v : 0;
  const char *p;
  if ((p = json_field(js, ml, "minID")) && *p == '"') b->min_len = b64dec(p + 1, b->min_id, 64);
  if ((p = json_field(js, ml, "maxID")) && *p == '"') b->max_len = b64dec(p + 1, b->max_id, 64);
  if ((p = json_field(js, ml, "startTime")) && *p == '"') b->start_unix = rfc3339_unix(p + 1);
  if ((p = json_field(js, ml, "endTime")) && *p == '"') b->end_unix = rfc3339_unix(p + 1);
  if ((p = json_field(js, ml, "blockID")) && *p == '"') parse_uuid(p + 1, b->block_id);
  free(meta);
  /* common.ValidateShardCount (bloom.go:88-93) */
  b->nbloom = b->bloom_shards ? b->bloom_shards : 10;
  b->bloom = (uint8_t **)calloc(b->nbloom, sizeof(uint8_t *));
  b->bloom_len = (size_t *)calloc(b->nbloom, sizeof(size_t));
  for (uint32_t i = 0; i < b->nbloom; i++) {
    char name[32];
    snprintf(name, sizeof name, "bloom-%u", i); /* common.BloomName (block.go:15-17) */
    rc = read_file(dir, name, &b->bloom[i], &b->bloom_len[i]);
    if (rc == ORC_NOT_FOUND) { b->bloom[i] = NULL; rc = ORC_OK; }
    if (rc) { orc_v2block_free(b); return rc; }
  }
  if ((rc = read_file(dir, "index", &b->index, &b->index_len)) ||
      (rc = read_file(dir, "data", &b->data, &b->data_len))) {
    if (rc == ORC_NOT_FOUND && b->index) rc = ORC_OK; /* data optional for id lookup */
    if (rc) { orc_v2block_free(b); return rc; }
  }
  *out = b;
  return ORC_OK;
}
void orc_v2block_free(orc_v2block *b) {
  if (!b) return;
  for (uint32_t i = 0; i < b->nbloom; i++) free(b->bloom[i]);
  free(b->bloom);
  free(b->bloom_len);
  free(b->index);
  free(b->data);
  free(b);
}
uint32_t orc_v2_shard_count(const orc_v2block *b) { return b->nbloom; }

/* willf/bloom Test after ReadFrom (vendor/github.com/willf/bloom/bloom.go:94-124,182-190,
 * 310-325; bitset.go:159-164,853-875): big-endian m, k, bitlen, words. */
static int bloom_test(const uint8_t *buf, size_t len, const uint8_t *id, size_t idl) {
  if (!buf || len < 24) return -ORC_CORRUPT;
  uint64_t m = be64(buf), k = be64(buf + 8), bitlen = be64(buf + 16);
  uint64_t nwords = (bitlen + 63) / 64; /* wordsNeeded */
  if (24 + nwords * 8 > len) return -ORC_CORRUPT;
  uint64_t h[4], t[2];
  orc_murmur3_128(id, idl, t);
  h[0] = t[0]; h[1] = t[1];
  uint8_t *tmp = (uint8_t *)malloc(idl + 1);
  memcpy(tmp, id, idl);
  tmp[idl] = 1;
  orc_murmur3_128(tmp, idl + 1, t);
  free(tmp);
  h[2] = t[0]; h[3] = t[1];
  if (m == 0) return -ORC_CORRUPT;
  for (uint64_t i = 0; i < k; i++) {
    uint64_t loc = (h[i % 2] + i * h[2 + (((i + (i % 2)) % 4) / 2)]) % m;
    if (loc >= bitlen) return 0;
    uint64_t w = be64(buf + 24 + (loc >> 6) * 8);
    if (!(w & (1ULL << (loc & 63)))) return 0;
  }
  return 1;
}
int orc_v2_bloom_test(const orc_v2block *b, const uint8_t *id, size_t idl) {
  /* ShardKeyForTraceID (bloom.go:83-85): int(FNV1_32(id)) % shardCount */
  uint32_t shard = orc_fnv1_32(id, idl) % b->nbloom;
  if (!b->bloom[shard]) return -ORC_NOT_FOUND;
  return bloom_test(b->bloom[shard], b->bloom_len[shard], id, idl);
}
int orc_v2_index_find(const orc_v2block *b, const uint8_t *id, size_t idl, int64_t *rec_idx, uint64_t *start,
                      uint32_t *length) {
  orc_index ix;
  index_init(&ix, b->index, b->index_len, b->index_page_size, b->total_records);
  int64_t i;
  int rc = index_find(&ix, id, idl, &i);
  if (!rc && i >= 0) {
    const uint8_t *r;
    int a = index_at(&ix, i, &r);
    if (a < 0) rc = -a;
    else { *start = le64(r + 16); *length = le32(r + 24); }
  }
  index_free(&ix);
  *rec_idx = rc ? -1 : i;
  return rc;
}
/* BackendBlock.find (backend_block.go:38-92) + PagedFinder.Find/findOne (finder_paged.go:35-111) */
int orc_v2_find(const orc_v2block *b, const uint8_t *id, size_t idl, uint8_t **out, size_t *out_len) {
  *out = NULL;
  *out_len = 0;
  int t = orc_v2_bloom_test(b, id, idl);
  if (t < 0) return -t;
  if (!t) return ORC_OK;
  int64_t ri;
  uint64_t start;
  uint32_t length;
  int rc = orc_v2_index_find(b, id, idl, &ri, &start, &length);
  if (rc || ri < 0) return rc;
  uint8_t *page;
  size_t pl;
  rc = data_read_page(b->data, b->data_len, b->enc, start, length, &page, &pl);
  if (rc) return rc;
  const uint8_t *cur = page, *oid, *obj;
  size_t cl = pl, objl;
  uint32_t oidl;
  for (;;) { /* iter.Next over bytes.NewReader(pages[0]) (finder_paged.go:89-108) */
    int u = unmarshal_from_reader(&cur, &cl, &oid, &oidl, &obj, &objl);
    if (u == 1) break;             /* io.EOF: nil, nil */
    if (u < 0) { rc = -u; break; } /* nil, err: only an id not found before it gets here */
    if (oidl == idl && memcmp(oid, id, idl) == 0) {
      *out = (uint8_t *)malloc(objl ? objl : 1);
      memcpy(*out, obj, objl);
      *out_len = objl;
      break;
    }
  }
  free(page);
  return rc;
}
/* includeBlock (tempodb/tempodb.go:492-511) */
int orc_v2_include_block(const orc_v2block *b, const uint8_t *id, uint32_t ts, uint32_t te, const uint8_t *bs,
                         const uint8_t *be) {
  if (bytes_compare(id, 16, b->min_id, b->min_len) == -1 || bytes_compare(id, 16, b->max_id, b->max_len) == 1)
    return 0;
  if (ts != 0 && te != 0)
    if (b->start_unix >= (int64_t)te || b->end_unix <= (int64_t)ts) return 0;
  if (bs && be)
    if (bytes_compare(b->block_id, 16, bs, 16) == -1 || bytes_compare(b->block_id, 16, be, 16) == 1) return 0;
  return 1;
}

typedef struct lk_arg {
  orc_v2block *const *blocks;
  uint32_t nblocks;
  const uint8_t (*ids)[16];
  uint64_t lo, hi;
  uint32_t ts, te;
  const uint8_t *bs, *be;
  orc_hit *h;
  uint64_t n, cap;
  int rc;
} lk_arg;
static void *lk_main(void *a) {
  lk_arg *t = (lk_arg *)a;
  orc_index *ix = (orc_index *)calloc(t->nblocks, sizeof(orc_index));
  for (uint32_t b = 0; b < t->nblocks; b++)
    index_init(&ix[b], t->blocks[b]->index, t->blocks[b]->index_len, t->blocks[b]->index_page_size,
               t->blocks[b]->total_records);
  for (uint64_t i = t->lo; i < t->hi; i++) {
    for (uint32_t b = 0; b < t->nblocks; b++) {
      const orc_v2block *blk = t->blocks[b];
      if (!orc_v2_include_block(blk, t->ids[i], t->ts, t->te, t->bs, t->be)) continue;
      int bt = orc_v2_bloom_test(blk, t->ids[i], 16);
      if (bt < 0) { t->rc = -bt; continue; }
      if (!bt) continue;
      int64_t ri;
      int rc = index_find(&ix[b], t->ids[i], 16, &ri);
      if (rc) { t->rc = rc; continue; }
      if (ri < 0) continue;
      const uint8_t *r;
      if (index_at(&ix[b], ri, &r) <= 0) { t->rc = ORC_CORRUPT; continue; }
      if (t->n == t->cap) {
        t->cap = t->cap ? t->cap * 2 : 1024;
        t->h = (orc_hit *)realloc(t->h, t->cap * sizeof(orc_hit));
      }
      orc_hit *h = &t->h[t->n++];
      h->id_idx = (uint32_t)i;
      h->block_idx = b;
      h->record_idx = (int32_t)ri;
      h->record_start = le64(r + 16);
      h->record_length = le32(r + 24);
    }
  }
  for (uint32_t b = 0; b < t->nblocks; b++) index_free(&ix[b]);
  free(ix);
  return NULL;
}
int orc_lookup_ids(orc_v2block *const *blocks, uint32_t nblocks, const uint8_t (*ids)[16], uint64_t nids,
                   uint32_t ts, uint32_t te, const uint8_t *bs, const uint8_t *be, int nthreads, orc_hit **out,
                   uint64_t *nout) {
  if (nthreads < 1) nthreads = 1;
  lk_arg *a = (lk_arg *)calloc((size_t)nthreads, sizeof *a);
  pthread_t *th = (pthread_t *)calloc((size_t)nthreads, sizeof *th);
  uint64_t per = (nids + (uint64_t)nthreads - 1) / (uint64_t)nthreads;
  for (int t = 0; t < nthreads; t++) {
    a[t].blocks = blocks; a[t].nblocks = nblocks; a[t].ids = ids;
    a[t].lo = per * (uint64_t)t < nids ? per * (uint64_t)t : nids;
    a[t].hi = per * (uint64_t)(t + 1) < nids ? per * (uint64_t)(t + 1) : nids;
    a[t].ts = ts; a[t].te = te; a[t].bs = bs; a[t].be = be;
    pthread_create(&th[t], NULL, lk_main, &a[t]);
  }
  uint64_t total = 0;
  int rc = ORC_OK;
  for (int t = 0; t < nthreads; t++) {
    pthread_join(th[t], NULL);
    total += a[t].n;
    if (a[t].rc && !rc) rc = a[t].rc;
  }
  orc_hit *h = (orc_hit *)malloc((total + 1) * sizeof(orc_hit));
  uint64_t k = 0;
  for (int t = 0; t < nthreads; t++) {
    if (a[t].n) memcpy(h + k, a[t].h, a[t].n * sizeof(orc_hit));
    k += a[t].n;
    free(a[t].h);
  }
  free(a);
  free(th);
  *out = h;
  *nout = total;
  return rc;
}

/* ------------------------------------------------------------------------- */
/* WAL search blocks (StreamingSearchBlock)                                    */

/* Go flatbuffers Builder (vendor/github.com/google/flatbuffers/go/builder.go, v2.0.0):
 * the bytes grow toward the front; offsets are measured from the end. Only what
 * SearchEntryMutable.ToBytes needs (pkg/tempofb/search_entry_mutable.go:41-63). */
typedef struct gob {
  uint8_t *b;
  size_t cap, head;
  int minalign;
  uint32_t vt[8];
  int nvt;
  uint32_t obj_end;
  uint32_t *vts;
  size_t nvts, cvts;
  /* CreateSharedString's map */
  uint8_t **ssk;
  size_t *ssl;
  uint32_t *sso;
  size_t nss, css;
} gob;
static uint32_t gob_off(const gob *f) { return (uint32_t)(f->cap - f->head); } /* Offset() */
static void gob_grow(gob *f) {                                                  /* growByteBuffer */
  size_t nc = f->cap ? f->cap * 2 : 1;
  uint8_t *nb = (uint8_t *)calloc(nc, 1);
  if (f->cap) memcpy(nb + (nc - f->cap), f->b, f->cap);
  free(f->b);
  f->head += nc - f->cap;
  f->b = nb;
  f->cap = nc;
}
static void gob_prep(gob *f, int size, size_t extra) { /* Prep */
  if (size > f->minalign) f->minalign = size;
  size_t align = (size_t)(-(int64_t)(gob_off(f) + extra)) & (size_t)(size - 1);
  while (f->head <= align + (size_t)size + extra) gob_grow(f);
  for (size_t i = 0; i < align; i++) f->b[--f->head] = 0; /* Pad */
}
static void gob_place32(gob *f, uint32_t x) {
  f->head -= 4;
  memcpy(f->b + f->head, &x, 4);
}
static void gob_place16(gob *f, uint16_t x) {
  f->head -= 2;
  memcpy(f->b + f->head, &x, 2);
}
static void gob_prepend_uoff(gob *f, uint32_t off) { /* PrependUOffsetT */
  gob_prep(f, 4, 0);
  gob_place32(f, gob_off(f) - off + 4);
}
static void gob_prepend_voff(gob *f, uint16_t x) { /* PrependVOffsetT */
  gob_prep(f, 2, 0);
  gob_place16(f, x);
}
static uint32_t gob_start_vector(gob *f, int elem, size_t n, int align) {
  gob_prep(f, 4, (size_t)elem * n);
  gob_prep(f, align, (size_t)elem * n);
  return gob_off(f);
}
static uint32_t gob_end_vector(gob *f, size_t n) {
  gob_place32(f, (uint32_t)n);
  return gob_off(f);
}
static uint32_t gob_bytes(gob *f, const uint8_t *s, size_t l) { /* CreateString / CreateByteString */
  gob_prep(f, 4, l + 1);
  f->b[--f->head] = 0;
  f->head -= l;
  if (l) memcpy(f->b + f->head, s, l);
  return gob_end_vector(f, l);
}
static uint32_t gob_shared(gob *f, const uint8_t *s, size_t l) { /* CreateSharedString */
  for (size_t i = 0; i < f->nss; i++)
    if (f->ssl[i] == l && memcmp(f->ssk[i], s, l) == 0) return f->sso[i];
  uint32_t o = gob_bytes(f, s, l);
  if (f->nss == f->css) {
    f->css = f->css ? f->css * 2 : 64;
    f->ssk = (uint8_t **)realloc(f->ssk, f->css * sizeof(uint8_t *));
    f->ssl = (size_t *)realloc(f->ssl, f->css * sizeof(size_t));
    f->sso = (uint32_t *)realloc(f->sso, f->css * sizeof(uint32_t));
  }
  f->ssk[f->nss] = (uint8_t *)malloc(l ? l : 1);
  if (l) memcpy(f->ssk[f->nss], s, l);
  f->ssl[f->nss] = l;
  f->sso[f->nss++] = o;
  return o;
}
static void gob_start_object(gob *f, int n) {
  memset(f->vt, 0, sizeof f->vt);
  f->nvt = n;
  f->obj_end = gob_off(f);
}
static void gob_uoff_slot(gob *f, int o, uint32_t x) { /* PrependUOffsetTSlot(o, x, 0) */
  if (x == 0) return;
  gob_prepend_uoff(f, x);
  f->vt[o] = gob_off(f);
}
static void gob_u64_slot(gob *f, int o, uint64_t x) { /* PrependUint64Slot(o, x, 0) */
  if (x == 0) return;
  gob_prep(f, 8, 0);
  f->head -= 8;
  memcpy(f->b + f->head, &x, 8);
  f->vt[o] = gob_off(f);
}
static uint32_t gob_end_object(gob *f) { /* WriteVtable */
  gob_prep(f, 4, 0); /* PrependSOffsetT(0) (overwritten below with the vtable's offset) */
  gob_place32(f, gob_off(f) + 4u);
  uint32_t obj = gob_off(f);
  int n = f->nvt;
  while (n > 0 && f->vt[n - 1] == 0) n--;
  uint32_t existing = 0;
  for (size_t i = f->nvts; i-- > 0;) {
    const uint8_t *v2 = f->b + (f->cap - f->vts[i]);
    uint16_t v2len = le16(v2);
    if ((size_t)n * 2 != (size_t)v2len - 4) continue;
    int eq = 1;
    for (int k = 0; k < n && eq; k++) {
      uint16_t x = le16(v2 + 4 + 2 * k);
      if (x == 0 && f->vt[k] == 0) continue;
      if ((int32_t)x != (int32_t)obj - (int32_t)f->vt[k]) eq = 0;
    }
    if (eq) { existing = f->vts[i]; break; }
  }
  if (!existing) {
    for (int k = n - 1; k >= 0; k--) gob_prepend_voff(f, (uint16_t)(f->vt[k] ? obj - f->vt[k] : 0));
    gob_prepend_voff(f, (uint16_t)(obj - f->obj_end));
    gob_prepend_voff(f, (uint16_t)((n + 2) * 2));
    int32_t so = (int32_t)gob_off(f) - (int32_t)obj;
    memcpy(f->b + (f->cap - obj), &so, 4);
    if (f->nvts == f->cvts) {
      f->cvts = f->cvts ? f->cvts * 2 : 16;
      f->vts = (uint32_t *)realloc(f->vts, f->cvts * sizeof(uint32_t));
    }
    f->vts[f->nvts++] = gob_off(f);
  } else {
    f->head = f->cap - obj;
    int32_t so = (int32_t)existing - (int32_t)obj;
    memcpy(f->b + f->head, &so, 4);
  }
  return obj;
}
static void gob_free(gob *f) {
  for (size_t i = 0; i < f->nss; i++) free(f->ssk[i]);
  free(f->ssk); free(f->ssl); free(f->sso); free(f->vts); free(f->b);
}

/* a (key, value) string pair of a SearchDataMap */
typedef struct kvp {
  uint8_t *k, *v;
  size_t kl, vl;
} kvp;
static int bcmp_go(const uint8_t *a, size_t al, const uint8_t *b, size_t bl) { /* Go string < */
  size_t n = al < bl ? al : bl;
  int c = n ? memcmp(a, b, n) : 0;
  if (c) return c;
  return al < bl ? -1 : (al > bl ? 1 : 0);
}
static int kvp_cmp(const void *x, const void *y) {
  const kvp *a = (const kvp *)x, *b = (const kvp *)y;
  int c = bcmp_go(a->k, a->kl, b->k, b->kl);
  return c ? c : bcmp_go(a->v, a->vl, b->v, b->vl);
}
typedef struct kvset {
  kvp *p;
  size_t n, cap;
} kvset;
static void kvset_add(kvset *s, const uint8_t *k, size_t kl, const uint8_t *v, size_t vl) {
  if (s->n == s->cap) {
    s->cap = s->cap ? s->cap * 2 : 64;
    s->p = (kvp *)realloc(s->p, s->cap * sizeof(kvp));
  }
  kvp *e = &s->p[s->n++];
  e->k = (uint8_t *)malloc(kl ? kl : 1);
  e->v = (uint8_t *)malloc(vl ? vl : 1);
  if (kl) memcpy(e->k, k, kl);
  if (vl) memcpy(e->v, v, vl);
  e->kl = kl;
  e->vl = vl;
}
static void kvset_unique(kvset *s) { /* sorted, one copy of each pair (the map's semantics) */
  if (!s->n) return;
  qsort(s->p, s->n, sizeof(kvp), kvp_cmp);
  size_t w = 1;
  for (size_t i = 1; i < s->n; i++) {
    if (kvp_cmp(&s->p[i], &s->p[w - 1]) == 0) { free(s->p[i].k); free(s->p[i].v); continue; }
    s->p[w++] = s->p[i];
  }
  s->n = w;
}
static void kvset_free(kvset *s) {
  for (size_t i = 0; i < s->n; i++) { free(s->p[i].k); free(s->p[i].v); }
  free(s->p);
}
/* every (key, value) of an entry's tags (SearchEntry.Tags / KeyValues.Value loops) */
static void entry_pairs(const fbt *e, kvset *s) {
  uint16_t to = fb_offset(e, VT_ENTRY_TAGS);
  uint32_t nt = to ? fb_vector_len(e, to) : 0;
  for (uint32_t t = 0; t < nt; t++) {
    fbt kv;
    if (!tc_tag(e, VT_ENTRY_TAGS, t, &kv)) continue;
    uint32_t kl = 0;
    uint16_t ko = fb_offset(&kv, VT_KV_KEY);
    const uint8_t *k = ko ? fb_byte_vector(&kv, ko + kv.pos, &kl) : (const uint8_t *)"";
    uint16_t vo = fb_offset(&kv, VT_KV_VALUE);
    uint32_t vn = vo ? fb_vector_len(&kv, vo) : 0;
    for (uint32_t j = 0; j < vn; j++) {
      uint32_t vl = 0;
      const uint8_t *v = fb_byte_vector(&kv, fb_vector(&kv, vo) + 4 * j, &vl);
      kvset_add(s, k, kl, v, vl);
    }
  }
}
static int str_cmp_ptr(const void *x, const void *y) {
  const kvp *a = (const kvp *)x, *b = (const kvp *)y;
  return bcmp_go(a->v, a->vl, b->v, b->vl);
}
/* DataCombiner.Combine's SearchEntryMutable -> ToBytes: CreateByteString(id),
 * WriteSearchDataMap (keys sorted, writeKeyValues lowercases + sorts values, shared
 * strings), SearchEntry{id, start, end, tags} (searchdatamap.go:71-152). */
static uint8_t *combined_to_bytes(const uint8_t *id, size_t idl, kvset *tags, uint64_t st, uint64_t en, size_t *len) {
  gob f;
  memset(&f, 0, sizeof f);
  f.minalign = 1;
  uint32_t ido = gob_bytes(&f, id, idl);
  kvset_unique(tags); /* (key, value) sorted: keys ascending as sort.Strings(keys) */
  uint32_t *offs = (uint32_t *)calloc(tags->n + 1, sizeof(uint32_t));
  size_t nk = 0;
  for (size_t i = 0; i < tags->n;) {
    size_t j = i;
    while (j < tags->n && bcmp_go(tags->p[j].k, tags->p[j].kl, tags->p[i].k, tags->p[i].kl) == 0) j++;
    uint8_t *lk = (uint8_t *)malloc(3 * tags->p[i].kl + 1);
    size_t lkl = go_to_lower(tags->p[i].k, tags->p[i].kl, lk);
    kvp *vals = (kvp *)calloc(j - i, sizeof(kvp));
    for (size_t q = i; q < j; q++) {
      vals[q - i].v = (uint8_t *)malloc(3 * tags->p[q].vl + 1);
      vals[q - i].vl = go_to_lower(tags->p[q].v, tags->p[q].vl, vals[q - i].v);
    }
    qsort(vals, j - i, sizeof(kvp), str_cmp_ptr); /* sort.Strings(values) */
    uint32_t ko = gob_shared(&f, lk, lkl);
    uint32_t *vs = (uint32_t *)calloc(j - i, sizeof(uint32_t));
    for (size_t q = 0; q < j - i; q++) vs[q] = gob_shared(&f, vals[q].v, vals[q].vl);
    gob_start_vector(&f, 4, j - i, 4);
    for (size_t q = 0; q < j - i; q++) gob_prepend_uoff(&f, vs[q]);
    uint32_t vv = gob_end_vector(&f, j - i);
    gob_start_object(&f, 2);
    gob_uoff_slot(&f, 0, ko);
    gob_uoff_slot(&f, 1, vv);
    offs[nk++] = gob_end_object(&f);
    for (size_t q = 0; q < j - i; q++) free(vals[q].v);
    free(vals);
    free(vs);
    free(lk);
    i = j;
  }
  gob_start_vector(&f, 4, nk, 4);
  for (size_t q = 0; q < nk; q++) gob_prepend_uoff(&f, offs[q]);
  uint32_t tv = gob_end_vector(&f, nk);
  free(offs);
  gob_start_object(&f, 4);
  gob_uoff_slot(&f, 0, ido);
  gob_u64_slot(&f, 2, st);
  gob_u64_slot(&f, 3, en);
  gob_uoff_slot(&f, 1, tv);
  uint32_t root = gob_end_object(&f);
  gob_prep(&f, f.minalign, 4); /* Finish */
  gob_prepend_uoff(&f, root);
  *len = f.cap - f.head;
  uint8_t *out = (uint8_t *)malloc(*len);
  memcpy(out, f.b + f.head, *len);
  gob_free(&f);
  return out;
}

/* wal.ParseFilename (tempodb/wal/wal.go:179-219): blockID:tenant:version:encoding[:dataEncoding] */
static int wal_parse_name(const char *name, int *enc) {
  char buf[512];
  size_t n = strlen(name);
  if (n >= sizeof buf) return ORC_INVALID;
  memcpy(buf, name, n + 1);
  char *parts[6];
  int np = 0;
  char *p = buf;
  for (;;) {
    if (np == 6) return ORC_INVALID;
    parts[np++] = p;
    char *c = strchr(p, ':');
    if (!c) break;
    *c = 0;
    p = c + 1;
  }
  if (np != 4 && np != 5) return ORC_INVALID;
  if (strlen(parts[0]) != 36) return ORC_INVALID;
  for (int i = 0; i < 36; i++) {
    int dash = i == 8 || i == 13 || i == 18 || i == 23;
    if (dash ? parts[0][i] != '-' : !isxdigit((unsigned char)parts[0][i])) return ORC_INVALID;
  }
  if (!parts[1][0]) return ORC_INVALID;
  if (strcmp(parts[2], "v2") != 0) return ORC_UNSUPPORTED_ENCODING;
  *enc = parse_encoding(parts[3]);
  return *enc < 0 ? ORC_INVALID : ORC_OK;
}

int orc_wal_block_load(const char *path, orc_block **out) {
  const char *slash = strrchr(path, '/');
  int enc = -1;
  int rc = wal_parse_name(slash ? slash + 1 : path, &enc);
  if (rc) return rc;
  orc_block *b = (orc_block *)calloc(1, sizeof(*b));
  b->wal = 1;
  b->has_meta = 1;
  b->enc = enc;
  strcpy(b->version, "v2");
  FILE *f = fopen(path, "rb");
  if (!f) { free(b); return ORC_IO; }
  fseek(f, 0, SEEK_END);
  long l = ftell(f);
  fseek(f, 0, SEEK_SET);
  b->data = (uint8_t *)malloc(l > 0 ? (size_t)l : 1);
  b->data_len = l > 0 && fread(b->data, 1, (size_t)l, f) == (size_t)l ? (size_t)l : 0;
  fclose(f);
  *out = b;
  return ORC_OK;
}

typedef struct walrec {
  uint8_t *id, *obj;
  size_t idl, objl, order;
} walrec;
static int walrec_cmp(const void *x, const void *y) { /* common.SortRecords: bytes.Compare on ids */
  const walrec *a = (const walrec *)x, *b = (const walrec *)y;
  int c = bcmp_go(a->id, a->idl, b->id, b->idl);
  if (c) return c;
  return a->order < b->order ? -1 : (a->order > b->order ? 1 : 0);
}

/* newStreamingSearchBlockFromWALReplay (rescan_blocks.go:74-107) + ReplayWALAndGetRecords
 * (wal/replay.go:15-71) + StreamingSearchBlock.Search (streaming_search_block.go:118-175)
 * through its deduping iterator (iterator_deduping.go, data_combiner.go). */
static int wal_search(const orc_block *b, uint32_t bidx, const orc_pipeline *p, mlist *out, consume_fn consume,
                      void *cctx, int *quit) {
  if (b->enc != 0 && b->enc != 6) return ORC_UNSUPPORTED_ENCODING;
  walrec *recs = NULL;
  size_t nr = 0, cr = 0;
  kvset hdr;
  memset(&hdr, 0, sizeof hdr);
  uint64_t min_dur = 0, max_dur = 0;
  size_t off = 0;
  while (off < b->data_len) { /* a damaged page ends the replay (warning), records kept */
    if (b->data_len - off < 6) break;
    uint32_t total = le32(b->data + off);
    if (total < 6 || total > b->data_len - off) break;
    uint8_t *page;
    size_t pl;
    if (data_read_page(b->data, b->data_len, b->enc, off, total, &page, &pl)) break;
    const uint8_t *cur = page, *id, *obj;
    size_t cl = pl, objl;
    uint32_t idl;
    if (unmarshal_advance(&cur, &cl, &id, &idl, &obj, &objl) != 0 || cl != 0) { free(page); break; }
    /* handleObj: SearchBlockHeaderMutable.AddEntry (SearchBlockHeader_util.go:21-43) */
    fbt e = fb_root(obj, objl);
    entry_pairs(&e, &hdr);
    uint64_t dur = fb_u64(&e, VT_ENTRY_END) - fb_u64(&e, VT_ENTRY_START);
    if (min_dur == 0 || dur < min_dur) min_dur = dur;
    if (dur > max_dur) max_dur = dur;
    if (nr == cr) {
      cr = cr ? cr * 2 : 64;
      recs = (walrec *)realloc(recs, cr * sizeof(walrec));
    }
    walrec *r = &recs[nr];
    r->id = (uint8_t *)malloc(idl ? idl : 1);
    if (idl) memcpy(r->id, id, idl);
    r->idl = idl;
    r->obj = (uint8_t *)malloc(objl ? objl : 1);
    if (objl) memcpy(r->obj, obj, objl);
    r->objl = objl;
    r->order = nr++;
    free(page);
    off += total;
  }
  int rc = ORC_OK;
  if (nr == 0) goto done; /* RescanBlocks drops an empty WAL file: no block, nothing counted */
  kvset_unique(&hdr);
  /* MatchesBlock on the mutable header: durations, then SearchDataMap.Contains (exact) */
  int ok = 1;
  if (p->has_min && !(max_dur >= p->min_ns)) ok = 0;
  if (p->has_max && !(min_dur <= p->max_ns)) ok = 0;
  for (uint32_t t = 0; t < p->nterms && ok; t++) {
    kvp key = {p->k[t], p->v[t], p->kl[t], p->vl[t]};
    if (!bsearch(&key, hdr.p, hdr.n, sizeof(kvp), kvp_cmp)) ok = 0;
  }
  if (!ok) {
    out->met.blocks_skipped++;
    goto done;
  }
  out->met.blocks_inspected++;
  qsort(recs, nr, sizeof(walrec), walrec_cmp);
  uint64_t scan_pos = 0;
  for (size_t i = 0; i < nr;) {
    if (*quit) break; /* sr.Quit() before each entry */
    size_t j = i + 1;
    while (j < nr && bcmp_go(recs[j].id, recs[j].idl, recs[i].id, recs[i].idl) == 0) j++;
    uint8_t *obj = recs[i].obj, *comb = NULL;
    size_t objl = recs[i].objl;
    if (j - i > 1) { /* DataCombiner.Combine */
      kvset tags;
      memset(&tags, 0, sizeof tags);
      uint64_t st = 0, en = 0;
      const uint8_t *tid = NULL;
      uint32_t tidl = 0;
      for (size_t k = i; k < j; k++) {
        if (recs[k].objl == 0) continue;
        fbt e = fb_root(recs[k].obj, recs[k].objl);
        entry_pairs(&e, &tags);
        uint64_t s2 = fb_u64(&e, VT_ENTRY_START), e2 = fb_u64(&e, VT_ENTRY_END);
        if (s2 > 0 && (st == 0 || st > s2)) st = s2;
        if (e2 > 0 && e2 > en) en = e2;
        uint16_t io = fb_offset(&e, VT_ENTRY_ID);
        tidl = 0;
        tid = io ? fb_byte_vector(&e, io + e.pos, &tidl) : NULL;
      }
      comb = combined_to_bytes(tid ? tid : (const uint8_t *)"", tidl, &tags, st, en, &objl);
      kvset_free(&tags);
      obj = comb;
    }
    out->met.bytes_inspected += objl; /* :160-161 */
    out->met.traces_inspected += 1;
    fbt e = fb_root(obj, objl);
    if (pipeline_matches(p, &e)) {
      orc_match *m;
      rc = result_from_entry(&e, bidx, scan_pos, out, &m);
      if (!rc && consume && consume(cctx, m)) *quit = 1;
    }
    free(comb);
    scan_pos++;
    i = j;
    if (rc) break;
  }
done:
  for (size_t i = 0; i < nr; i++) { free(recs[i].id); free(recs[i].obj); }
  free(recs);
  kvset_free(&hdr);
  return rc;
}

/* ------------------------------------------------------------------------- */
/* live traces (modules/ingester/instance_search.go:83-130)                     */
int orc_live_block_load_mem(const uint8_t *bytes, const uint64_t *seg_off, uint64_t nsegs, const uint64_t *trace_seg,
                            uint32_t ntraces, orc_block **out) {
  if (nsegs && (!seg_off || !bytes)) return ORC_INVALID;
  if (!trace_seg || trace_seg[0] != 0 || trace_seg[ntraces] != nsegs) return ORC_INVALID;
  for (uint32_t t = 0; t < ntraces; t++)
    if (trace_seg[t] > trace_seg[t + 1]) return ORC_INVALID;
  for (uint64_t i = 0; i < nsegs; i++)
    if (seg_off[i] > seg_off[i + 1]) return ORC_INVALID;
  orc_block *b = (orc_block *)calloc(1, sizeof(*b));
  b->live = 1;
  b->has_meta = 1;
  strcpy(b->version, "v2");
  b->ntraces = ntraces;
  b->nsegs = nsegs;
  const uint64_t total = nsegs ? seg_off[nsegs] - seg_off[0] : 0;
  b->data = (uint8_t *)malloc(total ? total : 1);
  if (total) memcpy(b->data, bytes + seg_off[0], total);
  b->data_len = total;
  b->seg_off = (uint64_t *)malloc((nsegs + 1) * sizeof(uint64_t));
  for (uint64_t i = 0; i <= nsegs; i++) b->seg_off[i] = nsegs ? seg_off[i] - seg_off[0] : 0;
  b->trace_seg = (uint64_t *)malloc(((uint64_t)ntraces + 1) * sizeof(uint64_t));
  memcpy(b->trace_seg, trace_seg, ((uint64_t)ntraces + 1) * sizeof(uint64_t));
  *out = b;
  return ORC_OK;
}

/* searchLiveTraces: per trace (the caller's order = the ingester's map iteration),
 * sr.Quit() check, AddTraceInspected(1); per segment AddBytesInspected(len(s)) and
 * p.Matches(entry) on its own; the matching segments' results combined with
 * CombineSearchResults (tempodb/search/util.go:40-62); one AddResult per trace.
 * entry_idx = the trace's position. No block filter, no blocksInspected. */
static int live_search(const orc_block *b, uint32_t bidx, const orc_pipeline *p, mlist *out, consume_fn consume,
                       void *cctx, int *quit) {
  for (uint32_t t = 0; t < b->ntraces; t++) {
    if (*quit) break;
    out->met.traces_inspected += 1;
    uint64_t mi = UINT64_MAX; /* index of this trace's result in out->m */
    for (uint64_t sgi = b->trace_seg[t]; sgi < b->trace_seg[t + 1]; sgi++) {
      const uint8_t *seg = b->data + b->seg_off[sgi];
      const size_t sl = (size_t)(b->seg_off[sgi + 1] - b->seg_off[sgi]);
      out->met.bytes_inspected += sl;
      if (sl < 4) return ORC_CORRUPT; /* (entry.Reset panics on a buffer without a root offset) */
      fbt e = fb_root(seg, sl);
      if (!pipeline_matches(p, &e)) continue;
      if (mi == UINT64_MAX) {
        orc_match *m;
        int rc = result_from_entry(&e, bidx, t, out, &m);
        if (rc) return rc;
        mi = out->n - 1;
        continue;
      }
      /* CombineSearchResults(existing, GetSearchResultFromData(entry)) */
      orc_match *x = &out->m[mi];
      uint32_t il = 0;
      const uint8_t *tid = NULL;
      uint16_t io = fb_offset(&e, VT_ENTRY_ID);
      if (io) tid = fb_byte_vector(&e, io + e.pos, &il);
      if (il > 16) return ORC_CORRUPT;
      static const uint8_t zero[16];
      if (memcmp(x->id, zero, 16) == 0) { /* existing.TraceID == "" (an all-zero id trims to "") */
        memset(x->id, 0, 16);
        if (il) memcpy(x->id + 16 - il, tid, il);
        x->id_len = il;
      }
      uint32_t sl2, nl2;
      const uint8_t *sv = entry_get(&e, "root.service.name", &sl2);
      const uint8_t *nv = entry_get(&e, "root.name", &nl2);
      if (x->svc_len == 0 && sl2) { x->svc_off = ml_str(out, sv, sl2); x->svc_len = sl2; }
      x = &out->m[mi];
      if (x->name_len == 0 && nl2) { x->name_off = ml_str(out, nv, nl2); x->name_len = nl2; }
      x = &out->m[mi];
      const uint64_t st = fb_u64(&e, VT_ENTRY_START), en = fb_u64(&e, VT_ENTRY_END);
      const uint32_t dur = (uint32_t)((en - st) / 1000000ULL);
      if (x->start_ns > st) x->start_ns = st;
      if (x->duration_ms < dur) x->duration_ms = dur;
    }
    if (mi != UINT64_MAX && consume && consume(cctx, &out->m[mi])) *quit = 1;
  }
  return ORC_OK;
}

/* ------------------------------------------------------------------------- */
/* SearchTags / SearchTagValues                                                 */
typedef struct strset {
  kvset s; /* (string, "") pairs */
} strset;
static void ss_add(strset *s, const uint8_t *p, size_t n) { kvset_add(&s->s, p, n, (const uint8_t *)"", 0); }
static int ss_pack(strset *s, uint8_t **out, size_t *len, size_t *n) { /* sorted, unique, u32 len + bytes */
  kvset_unique(&s->s);
  size_t total = 0;
  for (size_t i = 0; i < s->s.n; i++) total += 4 + s->s.p[i].kl;
  uint8_t *b = (uint8_t *)malloc(total ? total : 1);
  size_t o = 0;
  for (size_t i = 0; i < s->s.n; i++) {
    uint32_t l = (uint32_t)s->s.p[i].kl;
    memcpy(b + o, &l, 4);
    if (l) memcpy(b + o + 4, s->s.p[i].k, l);
    o += 4 + l;
  }
  *out = b;
  *len = total;
  *n = s->s.n;
  kvset_free(&s->s);
  memset(s, 0, sizeof *s);
  return ORC_OK;
}
static uint64_t ss_bytes(strset *s) { /* util.MapSizeWithinLimit's sum over the set's keys */
  kvset_unique(&s->s);
  uint64_t t = 0;
  for (size_t i = 0; i < s->s.n; i++) t += s->s.p[i].kl;
  return t;
}
/* the mutable header of a WAL block: every (key, value) of every replayed page's entry
 * (SearchBlockHeaderMutable.AddEntry, SearchBlockHeader_util.go:21-43) */
static void wal_header_pairs(const orc_block *b, kvset *hdr) {
  size_t off = 0;
  while (off < b->data_len) {
    if (b->data_len - off < 6) break;
    uint32_t total = le32(b->data + off);
    if (total < 6 || total > b->data_len - off) break;
    uint8_t *page;
    size_t pl;
    if (data_read_page(b->data, b->data_len, b->enc, off, total, &page, &pl)) break;
    const uint8_t *cur = page, *id, *obj;
    size_t cl = pl, objl;
    uint32_t idl;
    if (unmarshal_advance(&cur, &cl, &id, &idl, &obj, &objl) != 0 || cl != 0) { free(page); break; }
    fbt e = fb_root(obj, objl);
    entry_pairs(&e, hdr);
    free(page);
    off += total;
  }
}
/* Tags of one searchable block into s: BackendSearchBlock.Tags (header keys,
 * backend_search_block.go:145-162), StreamingSearchBlock.Tags (mutable header keys,
 * streaming_search_block.go:97-105), live traces (every segment's keys,
 * instance_search.go:191-200). A backend block without search data: the header read
 * fails (ErrDoesNotExist) -> ORC_NOT_FOUND. */
static int block_tags(const orc_block *b, strset *s) {
  if (b->live) {
    for (uint64_t i = 0; i < b->nsegs; i++) {
      const size_t sl = (size_t)(b->seg_off[i + 1] - b->seg_off[i]);
      if (sl < 4) return ORC_CORRUPT;
      fbt e = fb_root(b->data + b->seg_off[i], sl);
      uint32_t nt = tc_len(&e, VT_ENTRY_TAGS);
      for (uint32_t j = 0; j < nt; j++) {
        fbt kv;
        tc_tag(&e, VT_ENTRY_TAGS, j, &kv);
        uint32_t kl;
        const uint8_t *k = kv_key(&kv, &kl);
        ss_add(s, k ? k : (const uint8_t *)"", kl);
      }
    }
    return ORC_OK;
  }
  if (b->wal) {
    if (b->enc != 0 && b->enc != 6) return ORC_UNSUPPORTED_ENCODING;
    kvset hdr;
    memset(&hdr, 0, sizeof hdr);
    wal_header_pairs(b, &hdr);
    for (size_t i = 0; i < hdr.n; i++) ss_add(s, hdr.p[i].k, hdr.p[i].kl);
    kvset_free(&hdr);
    return ORC_OK;
  }
  if (!b->has_meta) return ORC_NOT_FOUND;
  fbt h = fb_root(b->header, b->header_len);
  uint32_t nt = tc_len(&h, VT_HDR_TAGS);
  for (uint32_t j = 0; j < nt; j++) {
    fbt kv;
    tc_tag(&h, VT_HDR_TAGS, j, &kv);
    uint32_t kl;
    const uint8_t *k = kv_key(&kv, &kl);
    ss_add(s, k ? k : (const uint8_t *)"", kl);
  }
  return ORC_OK;
}
static void kv_values_into(const fbt *kv, strset *s) {
  uint32_t vn = kv_value_len(kv);
  for (uint32_t j = 0; j < vn; j++) {
    uint32_t vl;
    const uint8_t *v = kv_value(kv, j, &vl);
    ss_add(s, v ? v : (const uint8_t *)"", vl);
  }
}
/* TagValues: FindTag on the header (backend_search_block.go:164-181); the mutable
 * header's values of exactly that key (streaming_search_block.go:107-116); FindTag on
 * every live segment (instance_search.go:229-240). */
static int block_tag_values(const orc_block *b, const uint8_t *key, size_t kl, strset *s) {
  if (b->live) {
    for (uint64_t i = 0; i < b->nsegs; i++) {
      const size_t sl = (size_t)(b->seg_off[i + 1] - b->seg_off[i]);
      if (sl < 4) return ORC_CORRUPT;
      fbt e = fb_root(b->data + b->seg_off[i], sl), kv;
      if (find_tag(&e, VT_ENTRY_TAGS, key, kl, &kv)) kv_values_into(&kv, s);
    }
    return ORC_OK;
  }
  if (b->wal) {
    if (b->enc != 0 && b->enc != 6) return ORC_UNSUPPORTED_ENCODING;
    kvset hdr;
    memset(&hdr, 0, sizeof hdr);
    wal_header_pairs(b, &hdr);
    for (size_t i = 0; i < hdr.n; i++)
      if (hdr.p[i].kl == kl && (kl == 0 || memcmp(hdr.p[i].k, key, kl) == 0)) ss_add(s, hdr.p[i].v, hdr.p[i].vl);
    kvset_free(&hdr);
    return ORC_OK;
  }
  if (!b->has_meta) return ORC_NOT_FOUND;
  fbt h = fb_root(b->header, b->header_len), kv;
  if (find_tag(&h, VT_HDR_TAGS, key, kl, &kv)) kv_values_into(&kv, s);
  return ORC_OK;
}
int orc_block_tags(const orc_block *b, uint8_t **out, size_t *len, size_t *n) {
  strset s;
  memset(&s, 0, sizeof s);
  int rc = block_tags(b, &s);
  if (rc) { kvset_free(&s.s); return rc; }
  return ss_pack(&s, out, len, n);
}
int orc_block_tag_values(const orc_block *b, const uint8_t *key, size_t kl, uint8_t **out, size_t *len, size_t *n) {
  strset s;
  memset(&s, 0, sizeof s);
  int rc = block_tag_values(b, key, kl, &s);
  if (rc) { kvset_free(&s.s); return rc; }
  return ss_pack(&s, out, len, n);
}
/* instance.SearchTags (instance_search.go:187-215): live traces first, then every block
 * (WAL, then local: the caller's order); the first block error fails the request. */
int orc_search_tags(orc_block *const *blocks, uint32_t nblocks, uint8_t **out, size_t *len, size_t *n) {
  strset s;
  memset(&s, 0, sizeof s);
  for (int pass = 0; pass < 2; pass++)
    for (uint32_t i = 0; i < nblocks; i++) {
      if ((blocks[i]->live != 0) != (pass == 0)) continue;
      int rc = block_tags(blocks[i], &s);
      if (rc) { kvset_free(&s.s); return rc; }
    }
  return ss_pack(&s, out, len, n);
}
/* instance.SearchTagValues (instance_search.go:217-273): live traces, then the size check
 * (util.MapSizeWithinLimit: sum of value lengths < max_bytes, else an EMPTY response),
 * then every block and the check again. max_bytes < 0: no check. */
int orc_search_tag_values(orc_block *const *blocks, uint32_t nblocks, const uint8_t *key, size_t kl, int64_t max_bytes,
                          uint8_t **out, size_t *len, size_t *n) {
  strset s;
  memset(&s, 0, sizeof s);
  for (int pass = 0; pass < 2; pass++) {
    for (uint32_t i = 0; i < nblocks; i++) {
      if ((blocks[i]->live != 0) != (pass == 0)) continue;
      int rc = block_tag_values(blocks[i], key, kl, &s);
      if (rc) { kvset_free(&s.s); return rc; }
    }
    if (max_bytes >= 0 && !((int64_t)ss_bytes(&s) < max_bytes)) {
      kvset_free(&s.s);
      memset(&s, 0, sizeof s);
      return ss_pack(&s, out, len, n);
    }
  }
  return ss_pack(&s, out, len, n);
}

/* SearchEntryMutable{id, tags, start, end}.ToBytes through the builder restatement
 * above (cross-checks the engine's writer, which restates the same builder). */
int orc_entry_to_bytes(const uint8_t *id, size_t idl, uint64_t st, uint64_t en, uint32_t npairs,
                       const uint8_t *const *k, const uint32_t *kl, const uint8_t *const *v, const uint32_t *vl,
                       uint8_t **out, size_t *out_len) {
  kvset tags;
  memset(&tags, 0, sizeof tags);
  for (uint32_t i = 0; i < npairs; i++) kvset_add(&tags, k[i], kl[i], v[i], vl[i]);
  *out = combined_to_bytes(id, idl, &tags, st, en, out_len);
  kvset_free(&tags);
  return ORC_OK;
}

/* ------------------------------------------------------------------------- */
/* CPU columnar baseline (see tsg_oracle.h)                                    */
typedef struct ctab { /* interned byte strings -> dense ids (open addressing on xxhash64) */
  uint64_t *slot_h;
  uint32_t *slot_id; /* UINT32_MAX = empty */
  uint64_t cap, n;
  uint8_t *bytes;
  uint64_t blen, bcap;
  uint64_t *off; /* n + 1 */
  uint64_t ocap;
} ctab;
static void ctab_init(ctab *t) {
  memset(t, 0, sizeof *t);
  t->cap = 64;
  t->slot_h = (uint64_t *)calloc(t->cap, 8);
  t->slot_id = (uint32_t *)malloc(t->cap * 4);
  memset(t->slot_id, 0xff, t->cap * 4);
  t->ocap = 64;
  t->off = (uint64_t *)calloc(t->ocap, 8);
}
static void ctab_free(ctab *t) {
  free(t->slot_h);
  free(t->slot_id);
  free(t->bytes);
  free(t->off);
}
static uint32_t ctab_id(ctab *t, const uint8_t *s, size_t l) {
  if (t->n * 2 + 2 > t->cap) { /* grow */
    uint64_t nc = t->cap * 2;
    uint64_t *nh = (uint64_t *)calloc(nc, 8);
    uint32_t *ni = (uint32_t *)malloc(nc * 4);
    memset(ni, 0xff, nc * 4);
    for (uint64_t i = 0; i < t->cap; i++) {
      if (t->slot_id[i] == UINT32_MAX) continue;
      uint64_t j = t->slot_h[i] & (nc - 1);
      while (ni[j] != UINT32_MAX) j = (j + 1) & (nc - 1);
      nh[j] = t->slot_h[i];
      ni[j] = t->slot_id[i];
    }
    free(t->slot_h);
    free(t->slot_id);
    t->slot_h = nh;
    t->slot_id = ni;
    t->cap = nc;
  }
  uint64_t h = orc_xxhash64(s, l), j = h & (t->cap - 1);
  while (t->slot_id[j] != UINT32_MAX) {
    uint32_t id = t->slot_id[j];
    if (t->slot_h[j] == h && t->off[id + 1] - t->off[id] == l && memcmp(t->bytes + t->off[id], s, l) == 0) return id;
    j = (j + 1) & (t->cap - 1);
  }
  uint32_t id = (uint32_t)t->n++;
  if (t->blen + l > t->bcap) {
    while (t->blen + l > t->bcap) t->bcap = t->bcap ? 2 * t->bcap : 4096;
    t->bytes = (uint8_t *)realloc(t->bytes, t->bcap);
  }
  if (l) memcpy(t->bytes + t->blen, s, l);
  t->blen += l;
  if (t->n + 1 > t->ocap) {
    t->ocap *= 2;
    t->off = (uint64_t *)realloc(t->off, t->ocap * 8);
  }
  t->off[id + 1] = t->blen;
  t->slot_h[j] = h;
  t->slot_id[j] = id;
  return id;
}

typedef struct ckey {
  ctab sets;     /* value sets: values joined as [u32 len][bytes]... */
  uint32_t *col; /* per entry: set id or UINT32_MAX (key absent) */
} ckey;
struct orc_colblock {
  uint64_t n, cap;
  uint64_t *start, *end;
  ctab keys;
  ckey *k;
  uint32_t nk, kcap;
};

static void cb_grow(orc_colblock *c, uint64_t need) {
  if (need <= c->cap) return;
  uint64_t nc = c->cap ? c->cap : 4096;
  while (nc < need) nc *= 2;
  c->start = (uint64_t *)realloc(c->start, nc * 8);
  c->end = (uint64_t *)realloc(c->end, nc * 8);
  for (uint32_t i = 0; i < c->nk; i++) {
    c->k[i].col = (uint32_t *)realloc(c->k[i].col, nc * 4);
    memset(c->k[i].col + c->cap, 0xff, (nc - c->cap) * 4);
  }
  c->cap = nc;
}

int orc_colblock_build(const orc_block *b, orc_colblock **out) {
  orc_colblock *c = (orc_colblock *)calloc(1, sizeof *c);
  ctab_init(&c->keys);
  *out = c;
  if (b->wal || !b->has_meta || b->enc < 0) return b->wal ? ORC_INVALID : ORC_OK;
  orc_index ix;
  index_init(&ix, b->index, b->index_len, b->index_page_size, b->index_records);
  uint8_t *joined = NULL;
  size_t jcap = 0;
  int rc = ORC_OK;
  for (int64_t i = 0;; i++) {
    const uint8_t *rec;
    if (index_at(&ix, i, &rec) <= 0) break;
    uint8_t *page;
    size_t pl;
    rc = data_read_page(b->data, b->data_len, b->enc, le64(rec + 16), le32(rec + 24), &page, &pl);
    if (rc) break;
    const uint8_t *cur = page, *id, *obj;
    size_t cl = pl, objl;
    uint32_t idl;
    if (unmarshal_advance(&cur, &cl, &id, &idl, &obj, &objl) != 0) { free(page); rc = ORC_CORRUPT; break; }
    fbt pg = fb_root(obj, objl);
    uint16_t eo = fb_offset(&pg, VT_PAGE_ENTRIES);
    uint32_t ne = eo ? fb_vector_len(&pg, eo) : 0;
    cb_grow(c, c->n + ne);
    for (uint32_t j = 0; j < ne; j++) {
      fbt e = pg;
      e.pos = fb_indirect(&pg, fb_vector(&pg, eo) + j * 4);
      const uint64_t ei = c->n++;
      c->start[ei] = fb_u64(&e, VT_ENTRY_START);
      c->end[ei] = fb_u64(&e, VT_ENTRY_END);
      uint16_t to = fb_offset(&e, VT_ENTRY_TAGS);
      uint32_t nt = to ? fb_vector_len(&e, to) : 0;
      for (uint32_t t = 0; t < nt; t++) {
        fbt kv = e;
        kv.pos = fb_indirect(&e, fb_vector(&e, to) + t * 4);
        uint32_t kl = 0;
        uint16_t ko = fb_offset(&kv, 4);
        const uint8_t *kp = ko ? fb_byte_vector(&kv, kv.pos + ko, &kl) : NULL;
        uint32_t kid = ctab_id(&c->keys, kp ? kp : (const uint8_t *)"", kl);
        if (kid >= c->nk) { /* new key: a column of its own */
          if (kid >= c->kcap) {
            c->kcap = c->kcap ? 2 * c->kcap : 32;
            c->k = (ckey *)realloc(c->k, c->kcap * sizeof(ckey));
          }
          ctab_init(&c->k[kid].sets);
          c->k[kid].col = (uint32_t *)malloc(c->cap * 4);
          memset(c->k[kid].col, 0xff, c->cap * 4);
          c->nk = kid + 1;
        }
        if (c->k[kid].col[ei] != UINT32_MAX) continue; /* first table of the key (unique keys) */
        uint16_t vo = fb_offset(&kv, 6);
        uint32_t vn = vo ? fb_vector_len(&kv, vo) : 0;
        size_t jl = 0;
        for (uint32_t q = 0; q < vn; q++) {
          uint32_t vl = 0;
          const uint8_t *vp = fb_byte_vector(&kv, fb_vector(&kv, vo) + q * 4, &vl);
          if (jl + 4 + vl > jcap) {
            jcap = (jl + 4 + vl) * 2;
            joined = (uint8_t *)realloc(joined, jcap);
          }
          memcpy(joined + jl, &vl, 4);
          if (vl) memcpy(joined + jl + 4, vp, vl);
          jl += 4 + vl;
        }
        c->k[kid].col[ei] = ctab_id(&c->k[kid].sets, joined, jl);
      }
    }
    free(page);
  }
  free(joined);
  index_free(&ix);
  return rc;
}
void orc_colblock_free(orc_colblock *c) {
  if (!c) return;
  for (uint32_t i = 0; i < c->nk; i++) {
    ctab_free(&c->k[i].sets);
    free(c->k[i].col);
  }
  free(c->k);
  ctab_free(&c->keys);
  free(c->start);
  free(c->end);
  free(c);
}
uint64_t orc_colblock_entries(const orc_colblock *c) { return c->n; }

typedef struct cscan {
  const orc_colblock *c;
  const orc_pipeline *p;
  const uint32_t *const *col; /* per term */
  uint8_t *const *bm;         /* per term: set id -> match */
  uint64_t lo, hi, bidx, matches, hash;
} cscan;
static void *cscan_main(void *a) {
  cscan *s = (cscan *)a;
  const orc_pipeline *p = s->p;
  uint64_t m = 0, h = 0;
  for (uint64_t e = s->lo; e < s->hi; e++) {
    const uint64_t st = s->c->start[e], et = s->c->end[e];
    if (p->has_min && !((et - st) >= p->min_ns)) continue;
    if (p->has_max && !((et - st) <= p->max_ns)) continue;
    if (p->has_range) {
      uint32_t ss = (uint32_t)(st / 1000000000ULL), es = (uint32_t)(et / 1000000000ULL);
      if (!(p->start <= es && p->end >= ss)) continue;
    }
    uint32_t t = 0;
    for (; t < p->nterms; t++) {
      uint32_t x = s->col[t][e];
      if (x == UINT32_MAX || !s->bm[t][x]) break;
    }
    if (t < p->nterms) continue;
    m++;
    h += ((s->bidx << 32) | e) * 0x9E3779B97F4A7C15ULL;
  }
  s->matches = m;
  s->hash = h;
  return NULL;
}

int orc_columnar_search(orc_colblock *const *cbs, uint32_t n, const orc_request *req, int nthreads,
                        uint64_t *matches, uint64_t *hash) {
  orc_pipeline p;
  pipeline_new(req, &p);
  if (nthreads < 1) nthreads = 1;
  uint64_t m = 0, h = 0;
  for (uint32_t b = 0; b < n && !p.exhaustive; b++) {
    const orc_colblock *c = cbs[b];
    const uint32_t **col = (const uint32_t **)calloc(p.nterms + 1, sizeof(void *));
    uint8_t **bm = (uint8_t **)calloc(p.nterms + 1, sizeof(void *));
    int dead = 0;
    for (uint32_t t = 0; t < p.nterms && !dead; t++) { /* dictionary pass: value sets matching term t */
      uint32_t kid = UINT32_MAX;
      for (uint32_t k = 0; k < c->nk; k++)
        if (c->keys.off[k + 1] - c->keys.off[k] == p.kl[t] && memcmp(c->keys.bytes + c->keys.off[k], p.k[t], p.kl[t]) == 0)
          kid = k;
      if (kid == UINT32_MAX) { dead = 1; break; }
      const ctab *sets = &c->k[kid].sets;
      bm[t] = (uint8_t *)calloc(sets->n + 1, 1);
      for (uint64_t sidx = 0; sidx < sets->n; sidx++) {
        const uint8_t *q = sets->bytes + sets->off[sidx], *qe = sets->bytes + sets->off[sidx + 1];
        while (q < qe && !bm[t][sidx]) {
          uint32_t vl;
          memcpy(&vl, q, 4);
          bm[t][sidx] = (uint8_t)bytes_contains(q + 4, vl, p.v[t], p.vl[t]);
          q += 4 + vl;
        }
      }
      col[t] = c->k[kid].col;
    }
    if (!dead && c->n) {
      int nt = nthreads;
      if ((uint64_t)nt > c->n) nt = (int)c->n;
      cscan *sc = (cscan *)calloc((size_t)nt, sizeof *sc);
      pthread_t *th = (pthread_t *)calloc((size_t)nt, sizeof *th);
      for (int i = 0; i < nt; i++) {
        sc[i].c = c;
        sc[i].p = &p;
        sc[i].col = col;
        sc[i].bm = bm;
        sc[i].bidx = b;
        sc[i].lo = c->n * (uint64_t)i / (uint64_t)nt;
        sc[i].hi = c->n * (uint64_t)(i + 1) / (uint64_t)nt;
        pthread_create(&th[i], NULL, cscan_main, &sc[i]);
      }
      for (int i = 0; i < nt; i++) {
        pthread_join(th[i], NULL);
        m += sc[i].matches;
        h += sc[i].hash;
      }
      free(sc);
      free(th);
    }
    for (uint32_t t = 0; t < p.nterms; t++) free(bm[t]);
    free(bm);
    free(col);
  }
  pipeline_free(&p);
  *matches = m;
  *hash = h;
  return ORC_OK;
}
