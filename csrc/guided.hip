// JSON-mode guided decoding on the device: the byte-level pushdown automaton
// of hyperspot/engine/guided.py (JsonByteMachine) as per-row device state and
// two kernels that sit in the captured decode graph around the sampler.
//
// State is int32 [rows, 11] (GUIDED_WORDS in ops/torch_ref.py), one row per
// logits row, no indirection:
//   w[0]      mode, the numbers of GUIDED_MODES in ops/torch_ref.py:
//               0 value      1 value_first  2 key        3 key_first
//               4 colon      5 string       6 escape     7 hex
//               8 lit        9 num_minus   10 num_zero  11 num_int
//              12 num_dot   13 num_frac    14 num_esign 15 num_e
//              16 num_exp   17 end         18 DEAD
//             < 0 = not a guided row (padding rows, pass-through replays,
//             rows that did not ask): neither kernel touches such a row.
//   w[1]      bit 0      in_key
//             bits 1..3  hex_left (0..4)
//             bits 4..5  the literal in progress: 0 none, 1 true, 2 false,
//                        3 null
//             bits 6..8  how many of its bytes remain (0 = none in progress).
//             A remaining "e" is stored as true's, whichever literal it ends:
//             the host machine keeps the remaining bytes only, so this is
//             the one encoding that pack() of the same machine gives.
//   w[2]      nesting depth, 0..256
//   w[3..10]  256 stack bits, 1 = obj, 0 = arr; bit d-1 is the container at
//             depth d.  Bits at and above the depth are 0.
//
// The host machine's stack is unbounded; here '{' and '[' are not allowed at
// depth 256, so the output stays valid JSON and differs from the host's only
// past that depth.  DEAD is entered by guided_json_advance on a byte the
// state does not allow (the host raises ValueError there; behind the mask
// and with finite logits it cannot happen); it allows EOS only and is
// sticky.  Words outside the ranges above (an unknown mode, a depth outside
// 0..256, a literal that is not one) read as DEAD, so no word value makes
// either kernel index out of bounds: the only indexed accesses are the stack
// words, behind the depth check.
//
//   guided_json_mask     -inf on every token the row's state does not allow.
//   guided_json_advance  feeds the token each row has just sampled.
//
// Both read every per-row fact from device memory; their grids depend on the
// row count and the vocabulary alone.  Byte tokenizer: byte b is id b + 4,
// EOS is id 2, so ids >= 260 are never allowed.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int kWords = 11;
constexpr int kMaxDepth = 256;
constexpr int kByteIds = 4 + 256;                 // specials + byte ids
constexpr int kEos = 2;
constexpr unsigned short kNegInf = 0xff80u;       // bf16 -inf

constexpr int kMaskVecs = 4;                      // 8-logit vectors / thread
constexpr int kMaskChunk = 256 * kMaskVecs * 8;   // logits per workgroup

enum Mode : int {
  VALUE = 0, VALUE_FIRST, KEY, KEY_FIRST, COLON, STRING, ESCAPE, HEX, LIT,
  NUM_MINUS, NUM_ZERO, NUM_INT, NUM_DOT, NUM_FRAC, NUM_ESIGN, NUM_E, NUM_EXP,
  END, DEAD
};

struct State {
  int mode;
  int in_key, hex_left, lit, lit_n;
  int depth;
  int top;                       // -1 stack empty, 0 arr, 1 obj
};

DEV int lit_len(int lit) { return lit == 2 ? 4 : 3; }   // bytes after the first

// next byte of the literal with n bytes left: "rue" / "alse" / "ull"
DEV int lit_next(int lit, int n) {
  const unsigned int tail = lit == 1 ? 0x00727565u     // e u r
                          : lit == 2 ? 0x616c7365u     // e s l a
                                     : 0x00756c6cu;    // l l u
  return (int)((tail >> (8 * (n - 1))) & 0xffu);
}

// w[0] >= 0.  Anything out of range reads as DEAD.
DEV State load_state(const int* __restrict__ w) {
  State s;
  s.mode = w[0];
  const int f = w[1];
  s.in_key = f & 1;
  s.hex_left = (f >> 1) & 7;
  s.lit = (f >> 4) & 3;
  s.lit_n = (f >> 6) & 7;
  s.depth = w[2];
  s.top = -1;
  if (s.mode > DEAD || s.depth < 0 || s.depth > kMaxDepth) {
    s.mode = DEAD;
    s.depth = 0;
  }
  if (s.mode == LIT &&
      (s.lit == 0 || s.lit_n < 1 || s.lit_n > lit_len(s.lit)))
    s.mode = DEAD;
  if (s.depth > 0) {
    const int d = s.depth - 1;                     // 0..255
    s.top = (w[3 + (d >> 5)] >> (d & 31)) & 1;
  }
  return s;
}

DEV bool is_digit(int b) { return b >= '0' && b <= '9'; }
DEV bool is_exp(int b) { return b == 'e' || b == 'E'; }

DEV bool is_hex(int b) {
  return is_digit(b) || (b >= 'a' && b <= 'f') || (b >= 'A' && b <= 'F');
}

// may follow a completed value in this context
DEV bool end_byte(const State& s, int b) {
  if (s.top < 0) return false;
  return b == ',' || b == (s.top ? '}' : ']');
}

DEV bool value_start(const State& s, int b) {
  if (b == '{' || b == '[') return s.depth < kMaxDepth;
  return b == '"' || b == '-' || b == 't' || b == 'f' || b == 'n' ||
         is_digit(b);
}

// JsonByteMachine.allowed(), byte b in 0..255
DEV bool byte_ok(const State& s, int b) {
  switch (s.mode) {
    case VALUE:       return value_start(s, b);
    // a closer needs a container to close (always there in a state the
    // host machine can reach): pop() never sees depth 0
    case VALUE_FIRST: return value_start(s, b) || (b == ']' && s.top >= 0);
    case KEY:         return b == '"';
    case KEY_FIRST:   return b == '"' || (b == '}' && s.top >= 0);
    case COLON:       return b == ':';
    case STRING:      return b >= 0x20;
    case ESCAPE:      return b == '"' || b == '\\' || b == '/' || b == 'b' ||
                             b == 'f' || b == 'n' || b == 'r' || b == 't' ||
                             b == 'u';
    case HEX:         return is_hex(b);
    case LIT:         return b == lit_next(s.lit, s.lit_n);
    case NUM_MINUS:   return is_digit(b);
    case NUM_ZERO:    return b == '.' || is_exp(b) || end_byte(s, b);
    case NUM_INT:     return is_digit(b) || b == '.' || is_exp(b) ||
                             end_byte(s, b);
    case NUM_DOT:     return is_digit(b);
    case NUM_FRAC:    return is_digit(b) || is_exp(b) || end_byte(s, b);
    case NUM_ESIGN:   return is_digit(b);
    case NUM_E:       return is_digit(b) || b == '+' || b == '-';
    case NUM_EXP:     return is_digit(b) || end_byte(s, b);
    case END:         return end_byte(s, b);
    default:          return false;                // DEAD
  }
}

// the top-level value is closed (JsonByteMachine.done); DEAD may only stop
DEV bool eos_ok(const State& s) {
  if (s.mode == DEAD) return true;
  return s.top < 0 && (s.mode == END || s.mode == NUM_ZERO ||
                       s.mode == NUM_INT || s.mode == NUM_FRAC ||
                       s.mode == NUM_EXP);
}

DEV bool id_ok(const State& s, int id) {
  if (id >= kByteIds) return false;
  if (id >= 4) return byte_ok(s, id - 4);
  return id == kEos && eos_ok(s);
}

DEV void push(State& s, int* __restrict__ w, int obj) {
  const int d = s.depth;                           // < kMaxDepth: allowed
  if (obj) w[3 + (d >> 5)] |= 1 << (d & 31);
  s.depth = d + 1;
}

DEV void pop(State& s, int* __restrict__ w) {
  const int d = s.depth - 1;                       // depth >= 1: allowed
  w[3 + (d >> 5)] &= ~(1 << (d & 31));
  s.depth = d;
}

// JsonByteMachine._feed_end
DEV void feed_end(State& s, int* __restrict__ w, int b) {
  if (b == ',') {
    s.mode = s.top ? KEY : VALUE;
  } else {
    pop(s, w);
    s.mode = END;
  }
}

}  // namespace

// grid rows * chunks, chunks = ceil((vocab + 8) / kMaskChunk), the chunk
// index varying fastest, so the chunks of ONE row spread over the 8 XCDs
// (profiles/r09_penalties.md measured 5x for the other order).  Store-only:
// every id >= 260 becomes -inf, with 16-byte stores over the vectors that
// lie whole inside the row past id 260; the vectors that hold ids < 260, and
// the head and tail of a row off the 16-byte grid, are written one logit at
// a time, the disallowed ones only, so allowed logits keep their bits
// without ever being loaded.
__global__ __launch_bounds__(256) void guided_json_mask_kernel(
    bf16* __restrict__ logits, const int* __restrict__ state, int vocab,
    int chunks) {
  const int r = blockIdx.x / chunks;
  const int chunk = blockIdx.x - r * chunks;
  const int* w = state + (long)r * kWords;
  if (w[0] < 0) return;                            // before any logit access
  const State s = load_state(w);                   // uniform per workgroup
  unsigned short* row =
      reinterpret_cast<unsigned short*>(logits) + (long)r * vocab;

  const int a = (int)(((uintptr_t)row >> 1) & 7);  // row's offset in its vector
  uint4* base = reinterpret_cast<uint4*>(row - a);
  const int end = a + vocab;
  const int nvec = (end + 7) >> 3;
  const int v0 = chunk * (256 * kMaskVecs);
  const unsigned int nn = ((unsigned int)kNegInf << 16) | kNegInf;

  #pragma unroll
  for (int k = 0; k < kMaskVecs; ++k) {
    const int v = v0 + k * 256 + threadIdx.x;
    if (v >= nvec) break;
    const int j0 = v * 8;                          // in the aligned frame
    if (j0 >= a + kByteIds && j0 + 8 <= end) {
      base[v] = make_uint4(nn, nn, nn, nn);
      continue;
    }
    unsigned short* vec = reinterpret_cast<unsigned short*>(base + v);
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = j0 + i;
      if (j < a || j >= end) continue;             // the neighbouring row's
      if (!id_ok(s, j - a)) vec[i] = kNegInf;
    }
  }
}

// One thread per row: JsonByteMachine.feed_token.  Tokens outside 4..259
// (EOS among them) leave the state as it is.
__global__ __launch_bounds__(256) void guided_json_advance_kernel(
    int* __restrict__ state, const long* __restrict__ sampled, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  int* w = state + (long)r * kWords;
  if (w[0] < 0) return;
  const long t = sampled[r];
  if (t < 4 || t >= kByteIds) return;
  const int b = (int)t - 4;
  State s = load_state(w);
  if (!byte_ok(s, b)) {                            // DEAD itself included
    w[0] = DEAD;
    return;
  }
  const int m = s.mode;
  switch (m) {
    case VALUE:
    case VALUE_FIRST:
      if (m == VALUE_FIRST && b == ']') { pop(s, w); s.mode = END; }
      else if (b == '"') { s.in_key = 0; s.mode = STRING; }
      else if (b == '{') { push(s, w, 1); s.mode = KEY_FIRST; }
      else if (b == '[') { push(s, w, 0); s.mode = VALUE_FIRST; }
      else if (b == '-') s.mode = NUM_MINUS;
      else if (b == '0') s.mode = NUM_ZERO;
      else if (is_digit(b)) s.mode = NUM_INT;
      else {
        s.lit = b == 't' ? 1 : b == 'f' ? 2 : 3;
        s.lit_n = lit_len(s.lit);
        s.mode = LIT;
      }
      break;
    case KEY:
    case KEY_FIRST:
      if (b == '}') { pop(s, w); s.mode = END; }
      else { s.in_key = 1; s.mode = STRING; }
      break;
    case COLON:
      s.mode = VALUE;
      break;
    case STRING:
      if (b == '"') s.mode = s.in_key ? COLON : END;
      else if (b == '\\') s.mode = ESCAPE;
      break;
    case ESCAPE:
      if (b == 'u') { s.hex_left = 4; s.mode = HEX; }
      else s.mode = STRING;
      break;
    case HEX:
      s.hex_left -= 1;
      if (s.hex_left <= 0) { s.hex_left = 0; s.mode = STRING; }
      break;
    case LIT:
      s.lit_n -= 1;
      if (s.lit_n == 0) { s.lit = 0; s.mode = END; }
      else if (s.lit_n == 1 && s.lit == 2) s.lit = 1;    // "e": see the top
      break;
    case NUM_MINUS:
      s.mode = b == '0' ? NUM_ZERO : NUM_INT;
      break;
    case NUM_ZERO:
    case NUM_INT:
    case NUM_FRAC:
    case NUM_EXP:
      if (b == '.') s.mode = NUM_DOT;
      else if (is_exp(b) && m != NUM_EXP) s.mode = NUM_E;
      else if (is_digit(b) && m != NUM_ZERO) {}          // stay
      else { s.mode = END; feed_end(s, w, b); }          // closes the number
      break;
    case NUM_DOT:
      s.mode = NUM_FRAC;
      break;
    case NUM_E:
      s.mode = is_digit(b) ? NUM_EXP : NUM_ESIGN;
      break;
    case NUM_ESIGN:
      s.mode = NUM_EXP;
      break;
    default:                                             // END
      feed_end(s, w, b);
      break;
  }
  w[0] = s.mode;
  w[1] = s.in_key | (s.hex_left << 1) | (s.lit << 4) | (s.lit_n << 6);
  w[2] = s.depth;
}

int guided_words() { return kWords; }

void launch_guided_json_mask(bf16* logits, const int* state, long rows,
                             int vocab, hipStream_t stream) {
  if (rows <= 0) return;
  // one extra vector covers a row that starts off the 16-byte grid
  const int chunks = (vocab + 8 + kMaskChunk - 1) / kMaskChunk;
  guided_json_mask_kernel<<<dim3((unsigned)(rows * chunks)), 256, 0,
                            stream>>>(logits, state, vocab, chunks);
}

void launch_guided_json_advance(int* state, const long* sampled, long rows,
                                hipStream_t stream) {
  if (rows <= 0) return;
  guided_json_advance_kernel<<<dim3((unsigned)((rows + 255) / 256)), 256, 0,
                               stream>>>(state, sampled, (int)rows);
}
