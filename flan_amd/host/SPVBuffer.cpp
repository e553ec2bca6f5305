// SPVBuffer.cpp -- host/device mirrored sliding-DFT container (reference: src/flan/SPV/SPVBuffer.cpp).
#include "flan/SPVBuffer.h"

#include <utility>

namespace flan {

SPVBuffer::SPVBuffer() : format() {}
SPVBuffer::SPVBuffer( const Format & f ) : format( f ) {}

SPVBuffer SPVBuffer::adopt_device( const Format & f, std::shared_ptr<detail::DeviceBlock> block )
	{
	SPVBuffer out( f );
	out.mirror.adopt( std::move( block ) );
	return out;
	}

SPVBuffer SPVBuffer::copy() const
	{
	SPVBuffer out( format );
	out.mirror = mirror.copy( count() );
	return out;
	}

bool SPVBuffer::is_null() const
	{
	return get_sample_rate() <= 0 || count() == 0;
	}

void SPVBuffer::clear_buffer() { mirror.clear( count() ); }

MF SPVBuffer::get_MF( Channel c, Frame f, Bin b ) const { return get_buffer()[get_buffer_pos( c, f, b )]; }
MF & SPVBuffer::get_MF( Channel c, Frame f, Bin b ) { return get_buffer()[get_buffer_pos( c, f, b )]; }

} // namespace flan
