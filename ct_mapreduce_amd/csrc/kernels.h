// kernels.h — the hand-written HIP kernels of the library, gfx950 (CDNA4, wave64) only.  No MFMA anywhere: this path
// is byte/integer scan + hash work bounded by HBM bandwidth.
//
//   kernels/readers.h   GlobalReader, WinReader/C/S — per-lane 256-byte LDS windows, wave-cooperative fills
//   kernels/sha256.h    k_issuer_ids (issuer table: walk Chain[0], SHA-256(RawSubjectPublicKeyInfo)), k_sha256_one
//   kernels/meta_core.h the read-only side of the IssuerMetadata memo (slot layout, item hash, CRL-DP walk, the map's pre-check)
//   kernels/map.h       the map — map_one (walk + filters + record), k_map_winc (the map without the fused insert)
//   kernels/map_sweep.h k_map_tile / k_map_direct: the two baseline designs, CTMR_SWEEP builds only (libctmr_sweep.so)
//   kernels/reduce.h    the known-certificate table (8-byte index words + 64-byte key cells): index_upsert, k_insert /
//                       k_insert2 (settle_order), k_map_fused (THE dominant kernel: walk + key parse + filters + pass 1 of
//                       the insert from the walking lane's registers; the default), k_ec_resolve (the curve equation of EC
//                       keys, then their pass 1), k_resolve, k_scan_blocks, k_compact
//   kernels/exchange.h  k_key_blockcount / k_key_gather / k_keys_insert* / k_keys_resolve / k_apply_lost (owner-computes
//                       exchange), k_filter_interleave / k_bloom_probe / k_keys_lookup / k_bloom_apply (Bloom variant)
//   kernels/pem.h       k_pem_len, k_pem_encode
//   kernels/entries.h   k_decode_match (decode + first Chain[0] match round), k_chain0_match, k_entry_decode (sweep builds)
//   kernels/meta.h      k_meta_new
//   kernels/writeback.h k_wb_count / k_wb_place / k_wb_order / k_wb_gather (a super-batch's first sightings grouped, ordered and
//                       rebased per ticket, their bytes packed: the ingestion pipeline's write-back)
//   kernels/misc.h      k_fingerprint, k_set_op / k_sweep / k_rehash / k_arena_compact / k_build_pairs / k_list,
//                       k_synth_*
//   kernels/image.h     k_pairs_slots / k_known_export / k_known_count / k_known_pack / k_known_bloom (the known-certificate image)
//   kernels/lists.h     k_lists_count / k_lists_write (per-issuer known-serial lists as text), k_image_lists_count /
//                       k_image_lists_write (the same straight from an image's member records)
//   kernels/resp.h      k_image_resp_count / k_image_resp_write (an image's member records as the Redis protocol stream of SADD
//                       and EXPIREAT commands)
//   kernels/resp_parse.h k_resp_mark / k_resp_cuts / k_resp_resolve / k_resp_chain / k_resp_commands / k_resp_place (a Redis
//                       protocol stream of SADD and EXPIREAT commands as it lies → an image's member records)
//   kernels/crl.h       k_crl_head / CrlCand / k_crl_class / k_crl_place (DER CertificateLists as they lie → the revoked
//                       serials as a probe image's member records; the mark kernel over CrlCand, the cuts and the chain
//                       proof are resp_parse.h's; k_crl_head<true> /
//                       k_crl_chain / k_crl_class<true>: a finding per CRL, for ctmr_crl_probes_each*)
//   kernels/text_scan.h what the two text decoders below share: a text in segments read in 16-byte chunks, the wave's scan
//                       and report, the base64 decode of a tile; k_ej_tiles / k_ej_tile_list (both decoders launch them)
//   kernels/entries_json.h k_ej_quotes / k_ej_mark / k_ej_resp / k_ej_check / k_ej_decode (get-entries JSON bodies as they
//                       lie → the raw-entry batch: tokens by quote parity, the grammar by position, base64 → bytes;
//                       k_ej_drop / k_ej_gather: every body judged on its own, the bad ones left out)
//   kernels/pem_decode.h k_pd_mark / k_pd_fstart / k_pd_files / k_pd_check / k_pd_squeeze / k_pd_decode (PEM certificate files
//                       as they lie → a packed batch: armor lines by their dashes, the grammar by counts, base64 → bytes)
//   kernels/sort.h      k_sort_keys / k_sort_hist / k_sort_scatter / k_sort_heads / k_sort_regroup / k_sort_gather (the
//                       order inside a known-certificate set: a segmented radix sort of member records)
//   kernels/merge.h     k_merge_ascending / k_merge_unique / k_merge_first / k_merge_rank / k_merge_sets / k_merge_place
//                       (set algebra on known-certificate images: union, minus, intersect of canonical member records)
//   kernels/find.h      k_find_build / k_find_scan / k_find_finish (serials looked up in a known image whatever their
//                       expiration date: the probes in a hash table, the image streamed once against it)
//   kernels/split.h     k_split_mark / k_split_place / k_split_sets (a known image partitioned by a probe image: a flag
//                       per record against the find's table, then one stable compaction into the two results)
//   kernels/cascade.h   k_casc_insert / k_casc_test / k_casc_compact / k_casc_query (the CRLite filter cascade of a revoked /
//                       not-revoked image pair: Bloom layers hashed with SHA-256, the false positives compacted into lists)
// der_walk.h is the TBSCertificate walk every kernel above shares; spki_key.h the key inside SubjectPublicKeyInfo.
#pragma once
#include "kernels/readers.h"
#include "kernels/sha256.h"
#include "kernels/meta_core.h"
#include "kernels/map.h"
#ifdef CTMR_SWEEP
#include "kernels/map_sweep.h"
#endif
#include "kernels/reduce.h"
#include "kernels/exchange.h"
#include "kernels/pem.h"
#include "kernels/entries.h"
#include "kernels/meta.h"
#include "kernels/writeback.h"
#include "kernels/misc.h"
#include "kernels/image.h"
#include "kernels/lists.h"
#include "kernels/resp.h"
#include "kernels/resp_parse.h"
#include "kernels/crl.h"
#include "kernels/text_scan.h"
#include "kernels/entries_json.h"
#include "kernels/pem_decode.h"
#include "kernels/sort.h"
#include "kernels/merge.h"
#include "kernels/find.h"
#include "kernels/split.h"
#include "kernels/cascade.h"
