// engine/sets.inc — storage.RemoteCache set methods, expiry, per-issuer counts.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

// ------------------------------------------------------------------ RemoteCache set methods

extern "C++" {
namespace {

// The host-side store (the engine mutex is held): where a member lives that is not a device-table member.  A serials::
// key of a registered issuer counts towards host_issuer_counts.
bool host_insert(ctmr_engine* e, const std::string& key, const std::string& m) {
  const bool ins = e->hstore[key].insert(m).second;
  int32_t eh; uint32_t canon;
  if (ins && table_key(e, key.data(), key.size(), &eh, &canon)) e->host_issuer_counts[canon]++;
  return ins;
}
bool host_contains(ctmr_engine* e, const std::string& key, const std::string& m) {
  auto it = e->hstore.find(key);
  return it != e->hstore.end() && it->second.count(m) != 0;
}
bool host_erase(ctmr_engine* e, const std::string& key, const std::string& m) {
  auto it = e->hstore.find(key);
  if (it == e->hstore.end() || !it->second.erase(m)) return false;
  int32_t eh; uint32_t canon;
  if (table_key(e, key.data(), key.size(), &eh, &canon)) e->host_issuer_counts[canon]--;
  if (it->second.empty()) e->hstore.erase(it);
  return true;
}

// a device-table member: a serial that fits a key cell, under the serials:: key of a registered issuer
bool set_point(ctmr_engine* e, const char* key, size_t kl, size_t ml, int32_t* eh, uint32_t* canon) {
  return ml <= CTMR_MAX_SERIAL && table_key(e, key, kl, eh, canon);
}

// SetInsert (op 0), SetContains (1) or SetRemove (2) of one member, the engine mutex held: a device-table member goes
// through point_op, anything else to the host-side store.  *out = 1: inserted / present / removed.
int set_op(ctmr_engine* e, int op, const char* key, size_t kl, const uint8_t* m, size_t ml, int* out) {
  int32_t eh; uint32_t canon;
  if (set_point(e, key, kl, ml, &eh, &canon)) return point_op(e, op, eh, canon, m, ml, out);
  const std::string k(key, kl), mem((const char*)m, ml);
  *out = op == 0 ? host_insert(e, k, mem) : op == 1 ? host_contains(e, k, mem) : host_erase(e, k, mem);
  return CTMR_OK;
}
int set_op(ctmr_engine* e, int op, const std::string& key, const std::string& m, int* out) {
  return set_op(e, op, key.data(), key.size(), (const uint8_t*)m.data(), m.size(), out);
}

}  // namespace
}  // extern "C++"

int ctmr_set_insert(ctmr_engine* e, const char* key, size_t kl, const uint8_t* m, size_t ml, int* was_new) {
  if (!e || !key || (ml && !m) || !was_new) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return set_op(e, 0, key, kl, m, ml, was_new);
}

int ctmr_set_contains(ctmr_engine* e, const char* key, size_t kl, const uint8_t* m, size_t ml, int* present) {
  if (!e || !key || (ml && !m) || !present) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return set_op(e, 1, key, kl, m, ml, present);
}

int ctmr_set_remove(ctmr_engine* e, const char* key, size_t kl, const uint8_t* m, size_t ml, int* removed) {
  if (!e || !key || (ml && !m) || !removed) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return set_op(e, 2, key, kl, m, ml, removed);
}

int ctmr_set_cardinality(ctmr_engine* e, const char* key, size_t kl, int64_t* n) {
  if (!e || !key || !n) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int64_t total = 0;
  auto it = e->hstore.find(std::string(key, kl));
  if (it != e->hstore.end()) total += (int64_t)it->second.size();
  int32_t eh; uint32_t canon;
  if (table_key(e, key, kl, &eh, &canon)) {
    uint64_t c;
    int r = pair_count(e, eh, canon, &c);
    if (r) return r;
    total += (int64_t)c;
  }
  *n = total;
  return CTMR_OK;
}

int ctmr_exists(ctmr_engine* e, const char* key, size_t kl, int* exists) {
  int64_t n;
  int r = ctmr_set_cardinality(e, key, kl, &n);
  if (r) return r;
  *exists = n > 0;
  return CTMR_OK;
}

int ctmr_set_members(ctmr_engine* e, const char* key, size_t kl, uint8_t* out, size_t cap, size_t* need, uint64_t* count) {
  if (!e || !key) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<std::string> v;
  auto it = e->hstore.find(std::string(key, kl));
  if (it != e->hstore.end()) v.assign(it->second.begin(), it->second.end());
  int32_t eh; uint32_t canon;
  if (table_key(e, key, kl, &eh, &canon)) {
    size_t capn = 1 << 12;
    for (;;) {
      int r = ensure(e, SC_MISC, capn * 48);
      if (r) return r;
      HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
      hipLaunchKernelGGL(k_list, dim3((unsigned)((e->nslots + 255) / 256)), dim3(256), 0, e->stream, e->tbl(),
                         (uint32_t)eh, canon, (uint8_t*)e->d_scratch[SC_MISC], (uint64_t)capn, e->d_count);
      unsigned long long cnt;
      HIPCHK(e, hipMemcpyAsync(&cnt, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
      if (cnt <= capn) {
        std::vector<uint8_t> buf(cnt * 48);
        if (cnt) HIPCHK(e, hipMemcpy(buf.data(), e->d_scratch[SC_MISC], cnt * 48, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; i++) {
          uint64_t l;
          memcpy(&l, &buf[i * 48], 8);
          v.emplace_back((const char*)&buf[i * 48 + 8], (size_t)l);
        }
        break;
      }
      capn = cnt + 64;
    }
  }
  std::sort(v.begin(), v.end());
  int rc;
  serialise(v, out, cap, need, count, &rc);
  return rc == CTMR_OK ? rc : fail(e, rc, "buffer too small");
}

int ctmr_keys(ctmr_engine* e, const char* pat, size_t pl, uint8_t* out, size_t cap, size_t* need, uint64_t* count) {
  if (!e || (pl && !pat)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  std::set<std::string> keys;
  for (auto& kv : e->hstore) if (!kv.second.empty()) keys.insert(kv.first);
  std::vector<PairRec> pr;
  int r = list_pairs(e, &pr);
  if (r) return r;
  for (auto& p : pr) keys.insert(make_key(e, p.exp_hour, p.canon));
  std::vector<std::string> v;
  for (auto& k : keys) if (glob_match(pat, pl, k.data(), k.size())) v.push_back(k);
  int rc;
  serialise(v, out, cap, need, count, &rc);
  return rc == CTMR_OK ? rc : fail(e, rc, "buffer too small");
}

int ctmr_expire_at(ctmr_engine* e, const char* key, size_t kl, int64_t t) {
  if (!e || !key) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  e->expiry[std::string(key, kl)] = t;
  return CTMR_OK;
}

int ctmr_expire_sweep(ctmr_engine* e, int64_t now, uint64_t* removed) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  uint64_t total = 0;
  // (1) every table key carries ExpireAt(expDate hour) (knowncertificates.go:98-104), unless
  //     overridden by an explicit later ExpireAt → handled in (2)
  std::vector<PairRec> pr;
  int r = list_pairs(e, &pr);
  if (r) return r;
  HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
  bool any_override = false;
  for (auto& p : pr)
    if (e->expiry.count(make_key(e, p.exp_hour, p.canon))) any_override = true;
  const unsigned blocks = (unsigned)((e->nslots + 255) / 256);
  e->pairs_dirty = true;
  if (!any_override) {
    hipLaunchKernelGGL(k_sweep, dim3(blocks), dim3(256), 0, e->stream, e->tbl(), 1, (long long)now, 0u, 0u,
                       e->issuer_counts, e->pairs, e->npairs - 1, e->d_count);
  } else {
    for (auto& p : pr) {
      auto it = e->expiry.find(make_key(e, p.exp_hour, p.canon));
      const int64_t t = it != e->expiry.end() ? it->second : (int64_t)p.exp_hour * 3600;
      if (t <= now)
        hipLaunchKernelGGL(k_sweep, dim3(blocks), dim3(256), 0, e->stream, e->tbl(), 0, 0ll, (uint32_t)p.exp_hour,
                           p.canon, e->issuer_counts, e->pairs, e->npairs - 1, e->d_count);
    }
  }
  unsigned long long cnt;
  HIPCHK(e, hipMemcpyAsync(&cnt, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  total += cnt;
  // (2) host-side keys
  for (auto it = e->hstore.begin(); it != e->hstore.end();) {
    int64_t t;
    bool has = false;
    auto ex = e->expiry.find(it->first);
    int32_t eh; uint32_t canon;
    const bool tk = table_key(e, it->first.data(), it->first.size(), &eh, &canon);
    if (ex != e->expiry.end()) { t = ex->second; has = true; }
    else if (tk) { t = (int64_t)eh * 3600; has = true; }
    if (has && t <= now) {
      total += it->second.size();
      if (tk) e->host_issuer_counts[canon] -= it->second.size();
      it = e->hstore.erase(it);
    } else {
      ++it;
    }
  }
  for (auto it = e->expiry.begin(); it != e->expiry.end();)
    it = it->second <= now ? e->expiry.erase(it) : std::next(it);
  if (removed) *removed = total;
  return CTMR_OK;
}

int ctmr_issuer_counts(ctmr_engine* e, uint64_t* out, uint32_t n) {
  if (!e || (n && !out)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const uint32_t have = (uint32_t)e->issuers.size();
  std::vector<unsigned long long> c(have);
  if (have) HIPCHK(e, hipMemcpy(c.data(), e->issuer_counts, (size_t)have * 8, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) {
    if (i >= have) { out[i] = 0; continue; }
    const uint32_t canon = e->issuers[i].canon;
    uint64_t v = c[canon];
    auto it = e->host_issuer_counts.find(canon);
    if (it != e->host_issuer_counts.end()) v += it->second;
    out[i] = e->issuers[i].valid ? v : 0;
  }
  return CTMR_OK;
}

int ctmr_total_count(ctmr_engine* e, uint64_t* out) {
  if (!e || !out) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const uint32_t have = (uint32_t)e->issuers.size();
  std::vector<unsigned long long> c(have);
  if (have) HIPCHK(e, hipMemcpy(c.data(), e->issuer_counts, (size_t)have * 8, hipMemcpyDeviceToHost));
  uint64_t t = 0;
  for (uint32_t i = 0; i < have; i++) if (e->issuers[i].canon == i) t += c[i];
  for (auto& kv : e->host_issuer_counts) t += kv.second;
  *out = t;
  return CTMR_OK;
}

int ctmr_issuer_counts_device(ctmr_engine* e, void** d, uint32_t* n) {
  if (!e || !d) return CTMR_E_INVAL;
  *d = e->issuer_counts;
  if (n) *n = e->max_issuers;
  return CTMR_OK;
}

int ctmr_table_info_get(ctmr_engine* e, ctmr_table_info* out) {
  if (!e || !out) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  out->slots = e->nslots;
  out->occupied = e->occupied;
  out->arena_cells = e->arena_cap;
  out->arena_used = e->arena_used;
  out->rebuilds = e->rebuilds;
  out->arena_compactions = e->arena_compactions;
  out->arena_growths = e->arena_growths;
  out->reserved = 0;
  return CTMR_OK;
}

int ctmr_reset_known(ctmr_engine* e) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemsetAsync(e->index, 0, e->nslots * 8, e->stream));  // 8 bytes per slot; the cells need no clearing:
  e->arena_used = 0;                                                  // nothing points to them any more
  HIPCHK(e, hipMemsetAsync(e->pairs, 0, e->npairs * sizeof(PairSlot), e->stream));
  e->pairs_dirty = false;
  e->occupied = 0;
  HIPCHK(e, hipMemsetAsync(e->issuer_counts, 0, (size_t)e->max_issuers * 8, e->stream));
  for (auto it = e->hstore.begin(); it != e->hstore.end();)
    it = it->first.compare(0, 9, "serials::") == 0 ? e->hstore.erase(it) : std::next(it);
  e->host_issuer_counts.clear();
  if (e->d_bloom) HIPCHK(e, hipMemsetAsync(e->d_bloom, 0, e->bloom_words * 8, e->stream));
  e->bloom_round_ref0 = ~0ull;
  return CTMR_OK;
}
