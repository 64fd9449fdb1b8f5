// Host-side symbolic stage of the MT3 path: event tokens -> notes.
//
// Product code (not the oracle).  C++ re-design of what the reference does in
// pure Python per token:
//   event_codec.Codec.decode_event_index            mt3/event_codec.py:103-112
//   run_length_encoding.decode_events               mt3/run_length_encoding.py:371-423
//   note_sequences.decode_note_event / _onset_event mt3/note_sequences.py:284-387
//   note_sequences.flush_note_decoding_state        mt3/note_sequences.py:396-408
//   note_sequences.assign_instruments               mt3/note_sequences.py:72-84
//   metrics_utils.decode_and_combine_predictions    mt3/metrics_utils.py:59-116
// Design: one pass over a flat token buffer with a prefix-offset codec table, an
// insertion-ordered active-note list (the reference relies on Python dict order
// when it ends un-tied notes and when it flushes), and "invalid event" signalled
// by a bool instead of exceptions.  All times are doubles evaluated with the
// reference's own expressions (start + steps / steps_per_second), so they are
// bit-identical; build with -ffp-contract=off.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "mt3_hip.h"
#include "common.h"

namespace {

constexpr double kDefaultNoteDuration = 0.01;  // note_sequences.py:29
constexpr double kMinNoteDuration = 0.01;      // note_sequences.py:32
constexpr int kDefaultVelocity = 100;          // note_sequences.py:28
constexpr int kMaxMidiVelocity = 127;          // note_seq.MAX_MIDI_VELOCITY

struct CodecTable {
  double steps_per_second = 100.0;
  int n = 0;
  int type[8], lo[8], hi[8], start[9];
  int velocity_bins = 0;
  bool ok = false;

  explicit CodecTable(const mt3_codec* c) {
    if (!c || c->num_ranges < 1 || c->num_ranges > 8) return;
    if (c->ranges[0].type != MT3_EV_SHIFT || c->ranges[0].min_value != 0) return;
    n = c->num_ranges;
    steps_per_second = c->steps_per_second;
    int off = 0;
    for (int i = 0; i < n; ++i) {
      type[i] = c->ranges[i].type;
      lo[i] = c->ranges[i].min_value;
      hi[i] = c->ranges[i].max_value;
      if (hi[i] < lo[i]) return;
      for (int j = 0; j < i; ++j)
        if (type[j] == type[i]) return;  // event types must be unique (event_codec.py:59-61)
      start[i] = off;
      off += hi[i] - lo[i] + 1;
      if (type[i] == MT3_EV_VELOCITY) velocity_bins = hi[i] - lo[i];  // vocabularies.py:57-60
    }
    start[n] = off;
    ok = true;
  }
  int num_classes() const { return start[n]; }
  // false == the reference's ValueError('Unknown event index')
  bool decode(int64_t index, int* t, int* v) const {
    if (index < 0 || index >= start[n]) return false;
    int k = 0;
    while (index >= start[k + 1]) ++k;
    *t = type[k];
    *v = lo[k] + static_cast<int>(index - start[k]);
    return true;
  }
  bool encode(int t, int v, int* index) const {
    for (int k = 0; k < n; ++k)
      if (type[k] == t) {
        if (v < lo[k] || v > hi[k]) return false;
        *index = start[k] + v - lo[k];
        return true;
      }
    return false;
  }
};

struct Active {
  int pitch, program;
  double onset;
  int velocity;
  int64_t token;      // index of the onset's token in the caller's flat buffer (mt3_notes_decode_traced)
};

class NoteMachine {
 public:
  NoteMachine(int spec, const CodecTable& codec, bool keep_trace) : spec_(spec), codec_(codec), keep_trace_(keep_trace) {}

  void begin_segment() {
    if (spec_ == MT3_SPEC_TIES) {  // begin_tied_pitches_section
      tied_.clear();
      in_tie_section_ = true;
    }
  }

  // returns false where the reference raises ValueError (caller counts it invalid)
  // at_token: the index of the event in the caller's flat token buffer (kept with the notes it creates / ends)
  bool consume(double time, int type, int value, int64_t at_token) {
    if (spec_ == MT3_SPEC_ONSETS) {
      if (type != MT3_EV_PITCH) return false;
      mt3_note n{};
      n.start_time = time;
      n.end_time = time + kDefaultNoteDuration;
      n.pitch = value;
      n.velocity = kDefaultVelocity;
      notes.push_back(n);
      if (keep_trace_) trace.push_back({at_token, -1});
      total_time = std::max(total_time, time + kDefaultNoteDuration);
      return true;
    }
    if (time < current_time_) return false;
    current_time_ = time;
    switch (type) {
      case MT3_EV_PITCH: {
        const int prog = current_program_;
        const int at = find(value, prog);
        if (in_tie_section_) {
          if (at < 0) return false;
          for (const auto& t : tied_)
            if (t.first == value && t.second == prog) return false;
          tied_.emplace_back(value, prog);
        } else if (current_velocity_ == 0) {
          if (at < 0) return false;
          const Active a = active_[at];
          active_.erase(active_.begin() + at);
          emit(a.onset, time, value, a.velocity, prog, false, a.token, at_token);
        } else {
          if (at >= 0) {  // re-onset of a sounding note: end it, start a new one
            const Active a = active_[at];
            active_.erase(active_.begin() + at);
            emit(a.onset, time, value, a.velocity, prog, false, a.token, at_token);
          }
          active_.push_back(Active{value, prog, time, current_velocity_, at_token});
        }
        return true;
      }
      case MT3_EV_DRUM:
        if (current_velocity_ == 0) return false;
        emit(time, time + kDefaultNoteDuration, value, current_velocity_, 0, true, at_token, -1);
        return true;
      case MT3_EV_VELOCITY:
        // vocabularies.bin_to_velocity: int(127 * bin / num_bins), 0 stays 0
        current_velocity_ =
            value == 0 ? 0
                       : static_cast<int>(static_cast<double>(kMaxMidiVelocity * value) /
                                          static_cast<double>(codec_.velocity_bins));
        return true;
      case MT3_EV_PROGRAM:
        current_program_ = value;
        return true;
      case MT3_EV_TIE: {
        if (!in_tie_section_) return false;
        std::vector<Active> keep;
        for (const Active& a : active_) {
          bool is_tied = false;
          for (const auto& t : tied_) is_tied |= (t.first == a.pitch && t.second == a.program);
          if (is_tied) keep.push_back(a);
          else emit(a.onset, current_time_, a.pitch, a.velocity, a.program, false, a.token, at_token);
        }
        active_.swap(keep);
        in_tie_section_ = false;
        return true;
      }
      default:
        return false;
    }
  }

  void flush() {
    if (spec_ == MT3_SPEC_ONSETS) return;  // NoteOnsetEncodingSpec: flush = identity
    for (const Active& a : active_) current_time_ = std::max(current_time_, a.onset + kMinNoteDuration);
    for (const Active& a : active_) emit(a.onset, current_time_, a.pitch, a.velocity, a.program, false, a.token, -1);
    active_.clear();
    // assign_instruments: order of first appearance of a program, skipping 9
    std::vector<std::pair<int, int>> seen;
    for (mt3_note& n : notes) {
      if (n.is_drum) { n.instrument = 9; continue; }
      int found = -1;
      for (const auto& s : seen)
        if (s.first == n.program) found = s.second;
      if (found < 0) {
        const int k = static_cast<int>(seen.size());
        found = k < 9 ? k : k + 1;
        seen.emplace_back(n.program, found);
      }
      n.instrument = found;
    }
  }

  std::vector<mt3_note> notes;
  std::vector<std::array<int64_t, 2>> trace;      // keep_trace: per note, the tokens that started / ended it (-1: none)
  double total_time = 0.0;

 private:
  int find(int pitch, int program) const {
    for (size_t i = 0; i < active_.size(); ++i)
      if (active_[i].pitch == pitch && active_[i].program == program) return static_cast<int>(i);
    return -1;
  }
  void emit(double start, double end, int pitch, int velocity, int program, bool drum, int64_t on_token,
            int64_t end_token) {
    end = std::max(end, start + kMinNoteDuration);
    mt3_note n{};
    n.start_time = start;
    n.end_time = end;
    n.pitch = pitch;
    n.velocity = velocity;
    n.program = program;
    n.is_drum = drum ? 1 : 0;
    notes.push_back(n);
    if (keep_trace_) trace.push_back({on_token, end_token});
    total_time = std::max(total_time, end);
  }

  int spec_;
  const CodecTable& codec_;
  bool keep_trace_;
  double current_time_ = 0.0;
  int current_velocity_ = kDefaultVelocity;
  int current_program_ = 0;
  std::vector<Active> active_;              // insertion ordered, like the reference's dict
  std::vector<std::pair<int, int>> tied_;
  bool in_tie_section_ = false;
};

}  // namespace

extern "C" {

int mt3_build_codec(int32_t steps_per_second, int32_t max_shift_seconds, int32_t num_velocity_bins,
                    mt3_codec* out) {
  if (!out || steps_per_second <= 0 || max_shift_seconds <= 0 || num_velocity_bins < 1)
    return mt3::fail(MT3_ERR_INVALID, "mt3_build_codec: bad arguments");
  std::memset(out, 0, sizeof(*out));
  out->steps_per_second = steps_per_second;
  out->num_ranges = 6;
  const mt3_event_range r[6] = {
      {MT3_EV_SHIFT, 0, steps_per_second * max_shift_seconds},
      {MT3_EV_PITCH, 0, 127},
      {MT3_EV_VELOCITY, 0, num_velocity_bins},
      {MT3_EV_TIE, 0, 0},
      {MT3_EV_PROGRAM, 0, 127},
      {MT3_EV_DRUM, 0, 127}};
  for (int i = 0; i < 6; ++i) out->ranges[i] = r[i];
  return MT3_OK;
}

int mt3_codec_num_classes(const mt3_codec* c) {
  CodecTable t(c);
  if (!t.ok) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_num_classes: malformed codec");
  return t.num_classes();
}

int mt3_codec_decode_event(const mt3_codec* c, int32_t index, int32_t* type, int32_t* value) {
  CodecTable t(c);
  if (!t.ok || !type || !value) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_decode_event: malformed codec");
  int ty, v;
  if (!t.decode(index, &ty, &v)) return mt3::fail(MT3_ERR_INVALID, "Unknown event index");
  *type = ty;
  *value = v;
  return MT3_OK;
}

int mt3_codec_encode_event(const mt3_codec* c, int32_t type, int32_t value, int32_t* index) {
  CodecTable t(c);
  if (!t.ok || !index) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_encode_event: malformed codec");
  int idx;
  if (!t.encode(type, value, &idx)) return mt3::fail(MT3_ERR_INVALID, "event type/value not in codec");
  *index = idx;
  return MT3_OK;
}

int mt3_codec_token_mask(const mt3_codec* c, int32_t vocab, const int32_t* programs, int32_t n_programs,
                         int32_t allow_drums, uint32_t* h_mask) {
  CodecTable t(c);
  if (!t.ok) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_mask: malformed codec");
  if (!h_mask || vocab < 3 || (n_programs > 0 && !programs))
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_mask: null argument or vocab < 3");
  int pk = -1;
  for (int k = 0; k < t.n; ++k)
    if (t.type[k] == MT3_EV_PROGRAM) pk = k;
  if (n_programs >= 0 && pk < 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_mask: the codec has no program range");
  for (int i = 0; i < n_programs; ++i)
    if (programs[i] < t.lo[pk] || programs[i] > t.hi[pk])
      return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_mask: program outside the codec's range");
  const int words = (vocab + 31) / 32;
  for (int w = 0; w < words; ++w) h_mask[w] = 0xffffffffu;
  if (vocab % 32) h_mask[words - 1] = (1u << (vocab % 32)) - 1u;
  const auto forbid = [&](int k, int v) {                     // token id = 3 + event index (mt3_ids_to_tokens)
    const int id = 3 + t.start[k] + v - t.lo[k];
    if (id < vocab) h_mask[id >> 5] &= ~(1u << (id & 31));
  };
  for (int k = 0; k < t.n; ++k) {
    if (t.type[k] == MT3_EV_DRUM && !allow_drums)
      for (int v = t.lo[k]; v <= t.hi[k]; ++v) forbid(k, v);
    if (k == pk && n_programs >= 0)
      for (int v = t.lo[k]; v <= t.hi[k]; ++v) {
        bool listed = false;
        for (int i = 0; i < n_programs; ++i) listed = listed || programs[i] == v;
        if (!listed) forbid(k, v);
      }
  }
  return MT3_OK;
}

int mt3_codec_token_grammar(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t max_steps, mt3_token_grammar* out) {
  CodecTable t(c);
  if (!c || !out) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: null argument");
  if (!t.ok) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: malformed codec");
  if (spec < MT3_SPEC_ONSETS || spec > MT3_SPEC_TIES) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: bad spec");
  int pitch = -1, tie = -1, program = -1;
  for (int k = 0; k < t.n; ++k) {
    if (t.type[k] == MT3_EV_PITCH) pitch = k;
    if (t.type[k] == MT3_EV_TIE) tie = k;
    if (t.type[k] == MT3_EV_PROGRAM) program = k;
  }
  if (pitch < 0 || tie < 0 || program < 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: the codec needs a pitch, a tie and a program range");
  if (max_steps < 1) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: max_steps must be at least 1");
  // a time past the largest shift takes two shifts in a row in a canonical stream, which the rule forbids
  if (max_steps > t.hi[0])
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: max_steps exceeds the codec's largest shift");
  if (3 + t.num_classes() > vocab)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_token_grammar: the codec's ranges do not fit below vocab");
  const auto count = [&](int k) { return t.hi[k] - t.lo[k] + 1; };       // token id = 3 + event index (mt3_ids_to_tokens)
  out->shift_first = 3 + t.start[0];
  out->shift_count = count(0);
  out->max_steps = max_steps;
  out->tie_id = 3 + t.start[tie];
  out->program_first = 3 + t.start[program];
  out->program_count = count(program);
  out->pitch_first = 3 + t.start[pitch];
  out->pitch_count = count(pitch);
  out->with_ties = spec == MT3_SPEC_TIES ? 1 : 0;
  return MT3_OK;
}

int mt3_codec_note_grammar(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t max_steps, mt3_note_grammar* out) {
  if (!c || !out) return mt3::fail(MT3_ERR_INVALID, "mt3_codec_note_grammar: null argument");
  mt3_note_grammar n{};
  if (const int rc = mt3_codec_token_grammar(c, spec, vocab, max_steps, &n.g)) return rc;
  CodecTable t(c);
  int velocity = -1, drum = -1;
  for (int k = 0; k < t.n; ++k) {
    if (t.type[k] == MT3_EV_VELOCITY) velocity = k;
    if (t.type[k] == MT3_EV_DRUM) drum = k;
  }
  if (velocity < 0 || drum < 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_note_grammar: the codec needs a velocity and a drum range");
  if (t.lo[velocity] != 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_note_grammar: the codec's velocity range must start at 0");
  if (!n.g.with_ties)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_note_grammar: the note rule needs a spec with a tie section");
  if (n.g.program_count > MT3_NOTE_MAX_PROGRAMS || n.g.pitch_count > MT3_NOTE_MAX_PITCHES)
    return mt3::fail(MT3_ERR_INVALID, "mt3_codec_note_grammar: more than 128 programs or pitches");
  n.velocity_first = 3 + t.start[velocity];
  n.velocity_count = t.hi[velocity] - t.lo[velocity] + 1;
  n.drum_first = 3 + t.start[drum];
  n.drum_count = t.hi[drum] - t.lo[drum] + 1;
  *out = n;
  return MT3_OK;
}

int32_t mt3_note_grammar_table_words(const mt3_note_grammar* n) { return n ? mt3n_table_words(n) : 0; }
int32_t mt3_note_grammar_advance(const mt3_note_grammar* n, int32_t gram_before, int32_t note, uint32_t* held, int32_t tok) {
  return n && held ? mt3n_advance(n, gram_before, note, held, tok) : note;
}
int32_t mt3_note_grammar_allowed(const mt3_note_grammar* n, int32_t gram, int32_t note, const uint32_t* held, int32_t id) {
  return n && held ? mt3n_allowed(n, gram, note, held, id) : 1;
}

int32_t mt3_token_grammar_initial(const mt3_token_grammar* g) { return g ? mt3g_initial(g) : 0; }
int32_t mt3_token_grammar_advance(const mt3_token_grammar* g, int32_t state, int32_t tok) {
  return g ? mt3g_advance(g, state, tok) : state;
}
int32_t mt3_token_grammar_allowed(const mt3_token_grammar* g, int32_t state, int32_t id) {
  return g ? mt3g_allowed(g, state, id) : 1;
}
// the noise of temperature sampling (mt3s_*, include/mt3_hip.h) as the host computes it
uint32_t mt3_sampling_bits(uint64_t seed, uint64_t stream, int32_t t, int32_t id) { return mt3s_bits(seed, stream, t, id); }
float mt3_sampling_gumbel(uint32_t bits) { return mt3s_gumbel(bits); }

// the machine behind mt3_notes_decode (h_note_tokens == nullptr) and mt3_notes_decode_traced; `who` names the entry
// point in its error messages
static int notes_decode_impl(const std::string& who, const mt3_codec* c, int32_t spec, int32_t n_segments,
                             const int32_t* h_tokens, const int64_t* h_seg_offsets, const double* h_start_times,
                             const int32_t* h_has_max_time, const double* h_max_times, mt3_note* h_notes,
                             int64_t notes_capacity, int64_t* n_notes, int64_t* invalid_events, int64_t* dropped_events,
                             double* total_time, int64_t* h_note_tokens) {
  CodecTable codec(c);
  if (!codec.ok) return mt3::fail(MT3_ERR_INVALID, who + ": malformed codec");
  if (spec < MT3_SPEC_ONSETS || spec > MT3_SPEC_TIES || n_segments < 0 || !n_notes)
    return mt3::fail(MT3_ERR_INVALID, who + ": bad spec / arguments");
  if (n_segments > 0 && (!h_seg_offsets || !h_start_times))
    return mt3::fail(MT3_ERR_INVALID, who + ": null segment arrays");

  // sorted(predictions, key=start_time): stable
  std::vector<int> order(n_segments);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return h_start_times[a] < h_start_times[b]; });

  NoteMachine m(spec, codec, h_note_tokens != nullptr);
  int64_t invalid = 0, dropped = 0;
  for (int k = 0; k < n_segments; ++k) {
    const int s = order[k];
    m.begin_segment();
    bool has_max;
    double max_time = 0.0;
    if (h_has_max_time) {
      has_max = h_has_max_time[s] != 0;
      if (has_max) max_time = h_max_times[s];
    } else {
      has_max = k + 1 < n_segments;
      if (has_max) max_time = h_start_times[order[k + 1]];
    }
    const double start = h_start_times[s];
    const int64_t b = h_seg_offsets[s], e = h_seg_offsets[s + 1];
    if (e < b) return mt3::fail(MT3_ERR_INVALID, who + ": seg_offsets not monotone");
    int64_t steps = 0;
    double now = start;
    for (int64_t i = b; i < e; ++i) {
      int type, value;
      if (!codec.decode(h_tokens[i], &type, &value)) { ++invalid; continue; }
      if (type == MT3_EV_SHIFT) {
        steps += value;
        now = start + static_cast<double>(steps) / codec.steps_per_second;
        // `if max_time and cur_time > max_time`: None and 0.0 are both falsy
        if (has_max && max_time != 0.0 && now > max_time) { dropped += e - i; break; }
      } else {
        steps = 0;
        if (!m.consume(now, type, value, i)) ++invalid;
      }
    }
  }
  m.flush();
  *n_notes = static_cast<int64_t>(m.notes.size());
  if (invalid_events) *invalid_events = invalid;
  if (dropped_events) *dropped_events = dropped;
  if (total_time) *total_time = m.total_time;
  if (*n_notes > notes_capacity) return mt3::fail(MT3_ERR_CAPACITY, who + ": notes buffer too small");
  if (*n_notes > 0) {
    if (!h_notes) return mt3::fail(MT3_ERR_INVALID, who + ": null notes buffer");
    std::memcpy(h_notes, m.notes.data(), sizeof(mt3_note) * m.notes.size());
    if (h_note_tokens) std::memcpy(h_note_tokens, m.trace.data(), sizeof(int64_t) * 2 * m.trace.size());
  }
  return MT3_OK;
}


int mt3_notes_decode(const mt3_codec* c, int32_t spec, int32_t n_segments, const int32_t* h_tokens,
                     const int64_t* h_seg_offsets, const double* h_start_times,
                     const int32_t* h_has_max_time, const double* h_max_times,
                     mt3_note* h_notes, int64_t notes_capacity, int64_t* n_notes,
                     int64_t* invalid_events, int64_t* dropped_events, double* total_time) {
  return notes_decode_impl("mt3_notes_decode", c, spec, n_segments, h_tokens, h_seg_offsets, h_start_times, h_has_max_time,
                           h_max_times, h_notes, notes_capacity, n_notes, invalid_events, dropped_events, total_time, nullptr);
}

int mt3_notes_decode_traced(const mt3_codec* c, int32_t spec, int32_t n_segments, const int32_t* h_tokens,
                            const int64_t* h_seg_offsets, const double* h_start_times,
                            const int32_t* h_has_max_time, const double* h_max_times,
                            mt3_note* h_notes, int64_t notes_capacity, int64_t* n_notes,
                            int64_t* invalid_events, int64_t* dropped_events, double* total_time,
                            int64_t* h_note_tokens) {
  return notes_decode_impl("mt3_notes_decode_traced", c, spec, n_segments, h_tokens, h_seg_offsets, h_start_times,
                           h_has_max_time, h_max_times, h_notes, notes_capacity, n_notes, invalid_events, dropped_events,
                           total_time, h_note_tokens);
}

// ---- the target tokenizer on the host (the rule: include/mt3_hip.h, mt3t_*; the kernel: tokenize.hip)
int mt3_codec_tokenize_rule(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t granularity, mt3_tokenize_rule* out) {
  const std::string who = "mt3_codec_tokenize_rule: ";
  if (!c || !out) return mt3::fail(MT3_ERR_INVALID, who + "null argument");
  CodecTable t(c);
  if (!t.ok) return mt3::fail(MT3_ERR_INVALID, who + "malformed codec");
  if (spec != MT3_SPEC_NOTES && spec != MT3_SPEC_TIES)
    return mt3::fail(MT3_ERR_INVALID, who + "spec must be MT3_SPEC_NOTES or MT3_SPEC_TIES (onsets only has no offsets to encode)");
  if (granularity < MT3_GRANULARITY_FULL || granularity > MT3_GRANULARITY_FLAT)
    return mt3::fail(MT3_ERR_INVALID, who + "unknown granularity");
  int at[6] = {-1, -1, -1, -1, -1, -1};
  for (int k = 0; k < t.n; ++k)
    if (t.type[k] >= 0 && t.type[k] < 6) at[t.type[k]] = k;
  for (int type : {MT3_EV_PITCH, MT3_EV_VELOCITY, MT3_EV_TIE, MT3_EV_PROGRAM, MT3_EV_DRUM})
    if (at[type] < 0) return mt3::fail(MT3_ERR_INVALID, who + "the codec needs pitch, velocity, tie, program and drum ranges");
  for (int type : {MT3_EV_PITCH, MT3_EV_PROGRAM, MT3_EV_DRUM})
    if (t.lo[at[type]] != 0 || t.hi[at[type]] != 127)
      return mt3::fail(MT3_ERR_INVALID, who + "the codec's pitch, program and drum ranges must be 0 .. 127");
  if (t.lo[at[MT3_EV_VELOCITY]] != 0) return mt3::fail(MT3_ERR_INVALID, who + "the codec's velocity range must start at 0");
  if (3 + static_cast<int64_t>(t.num_classes()) > vocab)
    return mt3::fail(MT3_ERR_INVALID, who + "the codec's ranges do not fit below vocab");
  mt3_tokenize_rule r{};
  r.spec = spec;
  r.vocab = vocab;
  r.max_shift_steps = t.hi[0];
  r.shift_first = 3 + t.start[0];
  r.pitch_first = 3 + t.start[at[MT3_EV_PITCH]];
  r.velocity_first = 3 + t.start[at[MT3_EV_VELOCITY]];
  r.velocity_count = t.hi[at[MT3_EV_VELOCITY]] + 1;
  r.tie_id = 3 + t.start[at[MT3_EV_TIE]];
  r.program_first = 3 + t.start[at[MT3_EV_PROGRAM]];
  r.drum_first = 3 + t.start[at[MT3_EV_DRUM]];
  for (int p = 0; p < MT3_TOKENIZE_PROGRAMS; ++p)          // mt3/vocabularies.py:77-116, the token side of a granularity
    r.program_map[p] = granularity == MT3_GRANULARITY_FLAT ? -1 : granularity == MT3_GRANULARITY_MIDI_CLASS ? 8 * (p / 8) : p;
  if (const char* bad = mt3t_bad_rule(&r, 2)) return mt3::fail(MT3_ERR_INVALID, who + bad);
  *out = r;
  return MT3_OK;
}

int mt3_notes_tokenize(const mt3_tokenize_rule* r, const int32_t* h_step, const int32_t* h_pitch, const int32_t* h_program,
                       const int32_t* h_velbin, const int32_t* h_is_drum, const int32_t* h_note, int32_t n_events,
                       int32_t step_lo, int32_t step_hi, int32_t stride, int32_t* h_ids, int32_t* h_note_of,
                       uint8_t* h_is_onset, int32_t* h_length, int32_t* h_truncated) {
  const std::string who = "mt3_notes_tokenize: ";
  if (const char* bad = mt3t_bad_rule(r, stride)) return mt3::fail(MT3_ERR_INVALID, who + bad);
  if (n_events < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_events must not be negative");
  if (n_events > 0 && (!h_step || !h_pitch || !h_program || !h_velbin || !h_is_drum || !h_note))
    return mt3::fail(MT3_ERR_INVALID, who + "null event array");
  if (!h_ids || !h_note_of || !h_is_onset || !h_length || !h_truncated) return mt3::fail(MT3_ERR_INVALID, who + "null output");
  mt3t_row(r, h_step, h_pitch, h_program, h_velbin, h_is_drum, h_note, n_events, step_lo, step_hi, stride, h_ids, h_note_of,
           h_is_onset, h_length, h_truncated);
  return MT3_OK;
}

}  // extern "C"
