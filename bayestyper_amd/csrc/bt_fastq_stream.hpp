// The half of a FASTQ stream object that does not care how the data was compressed (bt_fastq_scan: BGZF blocks; bt_fastq_gz_scan: one long gzip member):
// the inflated bytes lie in st.d_raw behind the tail the call before left; they become reads text in st.d_text, and the record that is not whole waits in
// st.d_tail.  Of BgzfStream only the buffers, the tail and max_in_bytes are used here.  Implemented in bt_fastq.hip.
#pragma once
#include "bt_bgzf_stream.hpp"

namespace bt {

struct FastqText;   // the file's line counter, the decompressed offset and the parse's work arrays
FastqText *fastq_text_create();
void fastq_text_destroy(FastqText *ft);
// st.d_raw [raw] -> *d_text [*text_len] (st.d_text, which has room for raw bytes); a tail of more than 8 x st.max_in_bytes is refused.  Complete on return.
int fastq_text_slab(const char *who, BgzfStream &st, FastqText &ft, uint64_t raw, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);
// the carried tail judged as the file's end
int fastq_text_finish(const char *who, BgzfStream &st, FastqText &ft, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats);

}  // namespace bt
